""""existing callers compile and link unchanged".  The reference's own test programs
(tests/test_cross_correlation.c, test_pearson_coefficient.c there) call the two entry points of the path with arguments of
fixed C types; tests/golden/reference_callers.json records, per program, the headers it includes and those types.  A caller
with exactly those includes, argument types and result type is compiled against this repo's include/
(audiosync/audiosync.h:12-119, audiosync/cross_correlation.h:10-11,24-25) and linked against libaudiosync.so.
-Werror: a prototype that no longer accepts a caller's types (an incompatible pointer, a missing declaration) fails the build.
Compile + link only: running needs a GPU (tests/test_gpu_capi.py runs the reference's twelve known answers from C through
tests/c/kat_runner.c).  The programs land in a temporary directory."""
import json
import os
import shutil
import subprocess
import tempfile

import pytest

from util import asx, graft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "reference_callers.json")) as _f:
    CALLERS = json.load(_f)["callers"]


def caller_source(spec):
    """a C99 program that includes what the caller includes and makes each of its calls with arguments of the recorded types"""
    lines = ["#include <%s>" % h for h in spec["includes"]] + ["", "int main(void)", "{"]
    for k, call in enumerate(spec["calls"]):
        args = []
        for i, t in enumerate(call["args"]):
            name = "a%d_%d" % (k, i)
            if t.endswith("*"):
                lines.append("    static %s s%d_%d[8];" % (t[:-1].strip(), k, i))
                lines.append("    %s %s = s%d_%d;" % (t, name, k, i))
            else:
                lines.append("    %s %s = 8;" % (t, name))
            args.append(name)
        lines.append("    %s r%d = %s(%s);" % (call["returns"], k, call["function"], ", ".join(args)))
        lines.append("    (void)r%d;" % k)
    lines += ["    return 0;", "}", ""]
    return "\n".join(lines)


@pytest.mark.parametrize("rel", sorted(CALLERS))
def test_reference_test_program_compiles_and_links_against_this_library(rel):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    spec = CALLERS[rel]
    asx()  # builds libaudiosync.so / libaudiosync_hip.so if they are not there
    lib_dir = graft.PKG_DIR
    assert os.path.exists(os.path.join(lib_dir, "libaudiosync.so"))
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, os.path.basename(rel))
        with open(src, "w") as f:
            f.write(caller_source(spec))
        exe = os.path.join(tmp, "caller")
        # the flags of the reference's own build (CMakeLists.txt: C99, -Wall -Wextra) with ITS include directory replaced by ours
        cmd = ["gcc", "-std=gnu99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
               "-L", lib_dir, "-laudiosync", "-laudiosync_hip", "-lm", "-lpthread", "-Wl,-rpath," + lib_dir]
        p = subprocess.run(cmd, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        assert os.path.exists(exe)
        # the program binds the entry points of the path by name
        nm = subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout
        bound = {line.split()[-1].split("@")[0] for line in nm.splitlines() if line.strip()}
        for call in spec["calls"]:
            assert call["function"] in bound, nm
