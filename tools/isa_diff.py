#!/usr/bin/env python3
"""usage: tools/isa_diff.py [--renames <map>] <old libaudiosync_hip.so> <new libaudiosync_hip.so>
Per-kernel instruction streams of two builds of the library compared: the gfx950 code objects are taken out of each offload
bundle, disassembled with llvm-objdump (no addresses, no encodings, branch targets as labels) and split by kernel symbol.  Prints
how many kernels of the old build are identical, differ or are missing in the new one, and names the new kernels.  Needs no GPU:
build the parent commit and this one with hipcc --offload-arch=gfx950 and compare the two .so files.
--renames: a file of `old demangled name<TAB>new demangled name` lines (names as c++filt prints them, without the parameter list;
`#` starts a comment): a kernel of the old build that the map names is compared with the new build's kernel of the new name instead
of being reported MISSING / NEW.  Every renamed kernel and every kernel that differs gets a line with both sides' instruction
counts and resources (VGPRs, SGPRs, scratch, static LDS, kernarg size, from the code objects' metadata)."""
import os
import re
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/llvm/bin/llvm-objdump")
READELF = os.environ.get("LLVM_READELF", os.path.join(os.path.dirname(OBJDUMP), "llvm-readelf"))
RESOURCES = (("vgpr", "vgpr_count"), ("sgpr", "sgpr_count"), ("scratch", "private_segment_fixed_size"),
             ("lds", "group_segment_fixed_size"), ("kernarg", "kernarg_segment_size"))


def code_objects(path):
    data = open(path, "rb").read()
    out = []
    for m in re.finditer(re.escape(MAGIC), data):
        p = m.start()
        count = struct.unpack_from("<Q", data, p + 24)[0]
        q = p + 32
        for _ in range(count):
            off, size, tsz = struct.unpack_from("<QQQ", data, q)
            q += 24
            triple = data[q:q + tsz].decode()
            q += tsz
            if "gfx950" in triple and size:
                out.append(data[p + off:p + off + size])
    return out


def kernels(path):
    """{mangled name: (instruction list, {resource: value})}"""
    found, res = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, blob in enumerate(code_objects(path)):
            co = os.path.join(tmp, "k%d.co" % i)
            with open(co, "wb") as f:
                f.write(blob)
            txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", co], capture_output=True, text=True,
                                 check=True).stdout
            cur = None
            for line in txt.split("\n"):
                m = re.match(r"^(?:\S+ )?<(\S+)>:$", line)
                if m:
                    cur = m.group(1)
                    found.setdefault(cur, [])
                elif cur is not None and line.strip():
                    ins = re.sub(r"\s*//.*$", "", line.strip())
                    found[cur].append(re.sub(r"<\S+>", "<L>", ins))
            notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True, check=True).stdout
            for block in notes.split("  - .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", block).group(1)
                res[name] = {short: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1)) for short, key in RESOURCES}
    # what follows a kernel's last instruction up to the next symbol is alignment padding (s_nop / s_code_end runs, "..."): its
    # length depends on what the linker placed next, not on the kernel
    for v in found.values():
        while v and (v[-1].startswith("s_nop") or v[-1].startswith("s_code_end") or v[-1] == "..."):
            v.pop()
    return {k: (v, res.get(k, {})) for k, v in found.items() if k.startswith("_Z")}


def demangle(names):
    names = list(names)
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def short(demangled):
    """the name without its parameter list: `void k_x<Sched<600, 10, 10, 6>, 16>`, `k_y`"""
    return demangled.split("(")[0]


def main():
    args = sys.argv[1:]
    renames = {}
    if args[:1] == ["--renames"] and len(args) >= 2:
        for line in open(args[1]):
            line = line.rstrip("\n")
            if line and not line.startswith("#"):
                a, b = line.split("\t")
                renames[a] = b
        args = args[2:]
    if len(args) != 2:
        sys.exit(__doc__)
    old, new = kernels(args[0]), kernels(args[1])
    dn = demangle(set(old) | set(new))
    new_by_short = {short(dn[k]): k for k in new}
    # the new build's kernel that stands for each old one: its own name, or the one the map gives
    partner = {}
    for k in old:
        to = renames.get(short(dn[k]))
        partner[k] = new_by_short.get(to) if to is not None else (k if k in new else None)
    taken = set(partner.values())
    same = [k for k in old if partner[k] and new[partner[k]][0] == old[k][0]]
    differ = [k for k in old if partner[k] and new[partner[k]][0] != old[k][0]]
    missing = [k for k in old if not partner[k]]
    added = [k for k in new if k not in taken]
    renamed = [k for k in old if partner[k] and partner[k] != k]
    print("old kernels %d: identical %d, differ %d, missing %d; new kernels %d; renamed %d; %d instructions compared"
          % (len(old), len(same), len(differ), len(missing), len(added), len(renamed), sum(len(v[0]) for v in old.values())))
    kept = [k for k in old if partner[k] == k]
    print("kernels that keep their name: %d, of which differ %d" % (len(kept), len([k for k in kept if k in differ])))
    for tag, ks in (("MISSING", missing), ("NEW", added)):
        for k in ks:
            print(tag, short(dn[k])[:160])
    if renamed or differ:
        print("old name | new name | instructions old | new | instruction list | " + " | ".join(s + " old/new" for s, _ in RESOURCES))
    for k in sorted(set(renamed) | set(differ), key=lambda k: short(dn[k])):
        (io, ro), (ino, rn) = old[k], new[partner[k]]
        print(" | ".join([short(dn[k]), short(dn[partner[k]]), str(len(io)), str(len(ino)), "equal" if io == ino else "DIFFERS"]
                         + ["%s/%s" % (ro.get(s, "?"), rn.get(s, "?")) for s, _ in RESOURCES]))
    sys.exit(1 if differ or missing else 0)


if __name__ == "__main__":
    main()
