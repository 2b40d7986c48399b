"""Closure of the ctypes binding over include/lwpose.h (CPU only).

``_lib.lib()`` re-types every prototype of the header by hand as ``argtypes``.  The names are held against the header in
test_host_logic.py; this holds the types: the same number of parameters, and for each the same width class (32-bit integer,
64-bit integer, float, double, pointer).  An ``int`` declared ``c_int64``, or a ``double`` declared ``c_int``, is silent stack
corruption and fails here."""
import ctypes as C
import os
import re

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lwpose.h")

I32, I64, F32, F64, PTR = "int32", "int64", "float", "double", "pointer"
C_CLASS = {"int": I32, "unsigned": I32, "int64_t": I64, "size_t": I64, "float": F32, "double": F64, "lwp_handle": PTR}
CTYPES_CLASS = {C.c_int: I32, C.c_uint: I32, C.c_int64: I64, C.c_uint64: I64, C.c_size_t: I64, C.c_float: F32, C.c_double: F64,
                C.c_void_p: PTR, C.c_char_p: PTR}


def prototypes():
    """{name: (return type, [parameter spellings])} of every ``<ret> lwp_name(<params>);`` of the header."""
    with open(HEADER) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t]*?[\w*])\s*\b(lwp_\w+)\s*\(([^()]*)\)\s*;", text):
        params = " ".join(params.split())
        assert name not in out, name
        out[name] = (" ".join(ret.split()), [] if params in ("void", "") else [p.strip() for p in params.split(",")])
    return out


def c_class(param):
    """Width class of one parameter as the header spells it (``const int* n``, ``int64_t shape[4]``, ``double ratio``)."""
    if "*" in param or "[" in param:
        return PTR
    words = [w for w in param.split() if w != "const"]
    assert len(words) == 2 and words[0] in C_CLASS, param     # <type> <name>
    return C_CLASS[words[0]]


def ctypes_class(t):
    if t in CTYPES_CLASS:
        return CTYPES_CLASS[t]
    assert issubclass(t, (C._Pointer, C.Array)), t
    return PTR


def test_the_class_tables_hold_on_this_platform():
    for t, cls in CTYPES_CLASS.items():
        assert C.sizeof(t) == {I32: 4, I64: 8, F32: 4, F64: 8, PTR: C.sizeof(C.c_void_p)}[cls], t
    assert c_class("const float* const* outs") == PTR and c_class("int out_dims[4]") == PTR and c_class("lwp_handle h") == PTR
    assert c_class("unsigned flags") == I32 and c_class("size_t n") == I64 and c_class("const double x") == F64


def test_every_prototype_has_matching_argtypes():
    protos = prototypes()
    assert len(protos) >= 121, len(protos)
    assert set(_lib.EXPORTS) <= set(protos), sorted(set(_lib.EXPORTS) - set(protos))
    L = _lib.lib()
    bad = []
    for name, (ret, params) in sorted(protos.items()):
        fn = getattr(L, name)
        argtypes = list(fn.argtypes or [])
        if not params and not argtypes:
            continue                                       # a void parameter list may leave argtypes unset
        want = [c_class(p) for p in params]
        got = [ctypes_class(t) for t in argtypes]
        if want != got:
            bad.append("%s: header %s, argtypes %s" % (name, want, got))
    assert not bad, "\n".join(bad)


def test_every_non_int_return_type_has_a_restype():
    L = _lib.lib()
    seen = 0
    for name, (ret, _) in prototypes().items():
        fn = getattr(L, name)
        if ret == "int":
            assert fn.restype is C.c_int, name
            continue
        seen += 1
        assert "*" in ret, (name, ret)                    # the header returns int or a pointer
        assert fn.restype is not C.c_int and fn.restype is not None, name
        if "char" in ret:
            assert fn.restype is C.c_char_p, name
    assert seen >= 1                                      # lwp_last_error
