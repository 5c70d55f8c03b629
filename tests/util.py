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
# types among its template arguments (asx_internal.h: Selections, Inputs); k_pearson_prep, which keeps a kernel per form, has a
# suffix for it.
INVERSE = {"all": "AsxSelAll", "window": "AsxWin", "rows": "AsxWinRows", "topk": "AsxSelTopk<"}
SEED = {"seed": "AsxSelSeed", "rows": "AsxWinRows", "topk": "AsxSelTopkSeed"}
INPUTS = {"pitched": "AsxAtPitch", "listed": "AsxAtList"}
POLICY = {
    "k_inv_cols_r": dict(INVERSE, prune="AsxSelPrune<"),
    "k_inv_cols": INVERSE,
    "k_refine_pick": SEED,
    "k_finalize": SEED,
    "k_refine_dots": INPUTS,
    "k_pearson_partial": INPUTS,
}
SUFFIX = {
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
    prune (the inverse kernels), seed / rows / topk (the kernels that take the seed); inputs: pitched / listed (k_pearson_prep
    asked for a selection alone: pitched)."""
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
    want = family + SUFFIX[family][(selection, inputs or "pitched")]
    for name, rec in kernels.items():
        base, args = template_args(name)
        if base == want:
            out.setdefault(", ".join(args), []).append((None, rec))
    return out
