"""shared helpers for the test-suite"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import __graft_entry__ as graft  # noqa: E402


def asx():
    """the ctypes package over libaudiosync_hip.so (built on demand)"""
    if not os.path.exists(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so")):
        graft.build()
    return graft.load()


def have_gpu():
    try:
        return asx().device_count() > 0
    except Exception:
        return False


# How the kernel families spell "selection S, inputs I" in their demangled names.  A family that is one template names the policy
# type among its template arguments (asx_internal.h: Selections, Inputs); a family with a kernel per form has a suffix for it.
POLICY = {
    "k_inv_cols_r": {"all": "AsxSelAll", "window": "AsxWin", "rows": "AsxWinRows", "topk": "AsxSelTopk<", "prune": "AsxSelPrune<"},
    "k_refine_pick": {"seed": "AsxSelSeed", "rows": "AsxWinRows", "topk": "AsxSelTopkSeed"},
    "k_refine_dots": {"pitched": "AsxAtPitch", "listed": "AsxAtList"},
}
SUFFIX = {
    "k_inv_cols": {"all": "", "window": "_w", "rows": "_wp", "topk": "_wx"},
    "k_finalize": {"seed": "", "rows": "_p", "topk": "_x"},
    "k_pearson_partial": {"pitched": "", "listed": "_l"},
    "k_pearson_prep": {("seed", "pitched"): "", ("rows", "pitched"): "_p", ("topk", "pitched"): "_x",
                       ("seed", "listed"): "_l", ("rows", "listed"): "_pl", ("topk", "listed"): "_xl"},
}


def template_args(name):
    """("k_x", ["Sched<600, 10, 10, 6>", "16", ...]) of a demangled kernel name (no template: an empty list)"""
    head = name.split("(")[0]
    if head.startswith("void "):
        head = head[5:]
    if "<" not in head:
        return head, []
    base, rest = head.split("<", 1)
    rest = rest.rstrip()[:-1]
    args, depth, cur = [], 0, ""
    for ch in rest:
        depth += (ch == "<") - (ch == ">")
        if ch == "," and depth == 0:
            args.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return base, args + [cur.strip()]


def kernel_forms(kernels, family, selection=None, inputs=None):
    """The kernels "family F, selection S, inputs I" among {demangled name: record}: {the template arguments the family's forms
    share, as one string: [(the policy's own template argument or None, record), ...]}.  selection: all / window / rows / topk /
    prune (the inverse kernels), seed / rows / topk (the kernels that take the seed); inputs: pitched / listed."""
    out = {}
    if family in POLICY:
        want = POLICY[family][selection or inputs]
        for name, rec in kernels.items():
            base, args = template_args(name)
            hit = [i for i, a in enumerate(args) if a == want or (want.endswith("<") and a.startswith(want))]
            if base == family and hit:
                own = args[hit[0]][len(want):].rstrip(" >") if want.endswith("<") else None
                out.setdefault(", ".join(args[:hit[0]]), []).append((own, rec))
        return out
    table = SUFFIX[family]
    want = family + (table[(selection, inputs or "pitched")] if (selection, inputs or "pitched") in table else table[selection or inputs])
    for name, rec in kernels.items():
        base, args = template_args(name)
        if base == want:
            out.setdefault(", ".join(args), []).append((None, rec))
    return out
