#!/usr/bin/env python3
"""usage: tools/isa_diff.py <old libaudiosync_hip.so> <new libaudiosync_hip.so>
Per-kernel instruction streams of two builds of the library compared: the gfx950 code objects are taken out of each offload
bundle, disassembled with llvm-objdump (no addresses, no encodings, branch targets as labels) and split by kernel symbol.  Prints
how many kernels of the old build are identical, differ or are missing in the new one, and names the new kernels.  Needs no GPU:
build the parent commit and this one with hipcc --offload-arch=gfx950 and compare the two .so files."""
import os
import re
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/llvm/bin/llvm-objdump")


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
    found = {}
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
    # what follows a kernel's last instruction up to the next symbol is alignment padding (s_nop / s_code_end runs, "..."): its
    # length depends on what the linker placed next, not on the kernel
    for v in found.values():
        while v and (v[-1].startswith("s_nop") or v[-1].startswith("s_code_end") or v[-1] == "..."):
            v.pop()
    return {k: v for k, v in found.items() if k.startswith("_Z")}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    same = [k for k in old if new.get(k) == old[k]]
    differ = [k for k in old if k in new and new[k] != old[k]]
    missing = [k for k in old if k not in new]
    added = [k for k in new if k not in old]
    print("old kernels %d: identical %d, differ %d, missing %d; new kernels %d; %d instructions compared"
          % (len(old), len(same), len(differ), len(missing), len(added), sum(len(v) for v in old.values())))

    def name(k):
        return subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip() or k

    for tag, ks in (("DIFFERS", differ), ("MISSING", missing), ("NEW", added)):
        for k in ks:
            print(tag, name(k)[:160])
    sys.exit(1 if differ or missing else 0)


if __name__ == "__main__":
    main()
