"""The binding's signature table (hipxcorr.SIGNATURES) against the C prototypes: every function of the table exists in the built
library and has, parameter for parameter and in its return type, the ctypes kind of what include/audiosync/xcorr_hip.h declares
(the diagnostics outside the header: of what their extern "C" definitions under csrc/ state).  No device."""
import ctypes
import glob
import os
import re

import pytest

from util import ROOT, asx, graft

NAME = r"asx_[a-z0-9_]+"
SCALARS = {"size_t": ctypes.c_size_t, "int": ctypes.c_int, "long": ctypes.c_long, "int64_t": ctypes.c_int64,
           "uint64_t": ctypes.c_uint64, "double": ctypes.c_double}


def strip_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def split_params(params):
    params = " ".join(params.split())
    return [] if params in ("", "void") else [p.strip() for p in params.split(",")]


def header_prototypes():
    """{name: (return type, [parameter, ...])} of every `ret name(params);` of the public header"""
    text = strip_comments(open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read())
    found = re.findall(r"([A-Za-z_][A-Za-z0-9_ ]*?[ *]+)(%s)\s*\(([^()]*)\)\s*;" % NAME, text)
    return {name: (" ".join(ret.split()), split_params(params)) for ret, name, params in found}


def csrc_definitions():
    """{name: (return type, [parameter, ...])} of every `extern "C" ret asx_...(params) {` under csrc/"""
    out = {}
    for path in sorted(glob.glob(os.path.join(graft.PKG_DIR, "csrc", "*"))):
        if os.path.isfile(path) and path.endswith((".hip", ".cpp", ".c", ".h")):
            text = strip_comments(open(path).read())
            for ret, name, params in re.findall(r'extern\s+"C"\s+([A-Za-z_][A-Za-z0-9_ ]*?[ *]+)(%s)\s*\(([^()]*)\)\s*\{' % NAME, text):
                out[name] = (" ".join(ret.split()), split_params(params))
    return out


def c_kind(decl, is_return=False):
    """the ctypes kind of a C parameter or return type: "pointer", None (a void return) or the scalar's ctypes type"""
    decl = decl.strip()
    if "*" in decl or decl.endswith("]"):
        return "pointer"
    words = [w for w in re.findall(r"[A-Za-z_][A-Za-z0-9_]*", decl) if w != "const"]
    if not is_return and len(words) > 1:
        words = words[:-1]                      # the parameter's name
    ctype = " ".join(words)
    if is_return and ctype == "void":
        return None
    assert ctype in SCALARS, "a C type this test does not know: %r" % decl
    return SCALARS[ctype]


def ctypes_kind(t):
    if t is None:
        return None
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "pointer"
    return t


@pytest.fixture(scope="module")
def hipxcorr():
    asx()
    from audiosync_amd import hipxcorr
    return hipxcorr


def test_the_parsers_find_the_prototypes():
    """all of the header by the one expression (the names as tests/test_abi.py finds them), and the definitions of csrc/"""
    from test_abi import declared_symbols
    assert sorted(header_prototypes()) == declared_symbols("xcorr_hip.h")
    defs = csrc_definitions()
    assert set(header_prototypes()) <= set(defs) and len(defs) >= 80, len(defs)
    assert c_kind("const float *d_source") == c_kind("int radix[16]") == c_kind("asx_plan *", True) == "pointer"
    assert c_kind("size_t n") is ctypes.c_size_t and c_kind("const int64_t lo") is ctypes.c_int64
    assert c_kind("void", True) is None and c_kind("long", True) is ctypes.c_long


def test_the_header_part_of_the_table_is_the_header(hipxcorr):
    header = header_prototypes()
    assert sorted(hipxcorr.ABI_SYMBOLS) == sorted(header) and isinstance(hipxcorr.ABI_SYMBOLS, list)
    assert len(set(hipxcorr.ABI_SYMBOLS)) == len(hipxcorr.ABI_SYMBOLS)
    assert set(header) <= set(hipxcorr.SIGNATURES)
    # what the table holds beside the header is defined in csrc/ and declared nowhere in the header
    extra = set(hipxcorr.SIGNATURES) - set(header)
    assert extra and extra <= set(csrc_definitions()), sorted(extra - set(csrc_definitions()))


def test_every_signature_has_the_kinds_of_its_prototype(hipxcorr):
    protos = dict(csrc_definitions())
    protos.update(header_prototypes())          # the header is the contract where both state a function
    L = ctypes.CDLL(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so"))
    wrong = []
    for name, (restype, argtypes) in hipxcorr.SIGNATURES.items():
        assert hasattr(L, name), name
        assert name in protos, name
        ret, params = protos[name]
        if len(argtypes) != len(params):
            wrong.append((name, "count", len(argtypes), len(params)))
            continue
        if ctypes_kind(restype) != c_kind(ret, True):
            wrong.append((name, "return", restype, ret))
        for i, (t, decl) in enumerate(zip(argtypes, params)):
            if ctypes_kind(t) != c_kind(decl):
                wrong.append((name, i, t, decl))
    assert not wrong, wrong


def test_the_header_and_the_definitions_agree():
    """the kinds of a header prototype are those of its definition: the test above means the same thing for both parts"""
    defs = csrc_definitions()
    for name, (ret, params) in header_prototypes().items():
        d_ret, d_params = defs[name]
        assert c_kind(ret, True) == c_kind(d_ret, True), name
        assert [c_kind(p) for p in params] == [c_kind(p) for p in d_params], name


def test_lib_applies_the_table(hipxcorr):
    """lib() has set every function's restype and argtypes from the table, the zero-argument ones to []"""
    L = hipxcorr.lib()
    for name, (restype, argtypes) in hipxcorr.SIGNATURES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    for name in ("asx_device_count", "asx_current_device", "asx_last_error", "asx_abi_version"):
        assert hipxcorr.SIGNATURES[name][1] == []
