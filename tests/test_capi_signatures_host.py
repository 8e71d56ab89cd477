"""The ctypes table of bwt-merge_amd/capi.py against the prototypes of include/bwtm.h, and the binding's own helpers: a wrong entry of
SYMBOLS hands the library wrong arguments without any error.  Needs the header and the table only: no library, no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELEMENTS = {"uint8_t": ctypes.c_uint8, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
WIDTHS = {"int": "32", "uint32_t": "32", "uint64_t": "64", "long long": "64", "double": "double"}


def prototypes():
    """{name: (return type, [parameter, ...])} of include/bwtm.h as written, comments stripped as tests/test_c_abi.py strips them."""
    text = open(os.path.join(ROOT, "include", "bwtm.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    found = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(bwtm_[A-Za-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = [" ".join(p.split()) for p in params.split(",")]
        found[name] = (" ".join(ret.split()), [] if params == ["void"] else params)
    return found


def header_kind(param):
    """(width class, element type name or None) of one parameter (or return type) of the header."""
    if "*" in param or "[" in param or re.search(r"\bbwtm_\w+_fn\b", param):
        element = re.match(r"(?:const )?(\w+)", param).group(1)
        return "pointer", element if element in ELEMENTS else None
    by_value = re.fullmatch(r"(?:const )?(long long|\w+)(?: \w+)?", param).group(1)         # "type name", or the bare type of a result
    return WIDTHS[by_value], None


def binding_kind(t):
    """(width class, element ctypes type or None) of one argument (or result) type of the binding."""
    if t is ctypes.c_double:
        return "double", None
    if isinstance(t, type) and issubclass(t, ctypes._SimpleCData) and t._type_ in "iIlLqQ":
        return str(8 * ctypes.sizeof(t)), None
    pointer = getattr(t, "pointer", t)                                       # an array argument type names its plain pointer type
    assert t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(pointer, (ctypes._Pointer, ctypes._CFuncPtr)), t
    return "pointer", getattr(pointer, "_type_", None) if issubclass(pointer, ctypes._Pointer) else None


def test_every_bound_signature_matches_its_prototype(bwtm):
    declared = prototypes()
    assert len(bwtm.capi.SYMBOLS) >= 154
    for name, restype, argtypes in bwtm.capi.SYMBOLS:
        assert name in declared, name
        ret, params = declared[name]
        assert len(argtypes) == len(params), (name, len(argtypes), params)
        if ret == "void":
            assert restype is None, name
        else:
            assert restype is not None and binding_kind(restype)[0] == header_kind(ret)[0], (name, ret, restype)
        for i, (param, t) in enumerate(zip(params, argtypes)):
            want, element = header_kind(param)
            got, bound = binding_kind(t)
            assert got == want, (name, i, param, t)
            if element is not None and t is not ctypes.c_void_p:             # vp on purpose: the address may be a device's
                assert bound is ELEMENTS[element], (name, i, param, t)


def test_the_parser_reads_the_header_as_written():
    """The comparison is only as good as the parser: spot checks of what it makes of four kinds of prototypes."""
    declared = prototypes()
    assert declared["bwtm_last_error"] == ("const char*", [])
    assert declared["bwtm_find_approx_stats"] == ("int", ["uint64_t stats[4]"])
    assert declared["bwtm_tune"] == ("int", ["const char* key", "long long value"])
    assert len(declared["bwtm_merge_host_pipelined"][1]) == 11
    assert header_kind("uint64_t stats[4]") == ("pointer", "uint64_t") and header_kind("const uint8_t* data") == ("pointer", "uint8_t")
    assert header_kind("long long value") == ("64", None) and header_kind("uint32_t k") == ("32", None) and header_kind("int") == ("32", None)
    assert header_kind("bwtm_alloc_fn alloc") == ("pointer", None) and header_kind("const bwtm_index* index") == ("pointer", None)


@pytest.mark.parametrize("name, dtype, other", [("a_u8", np.uint8, np.int8), ("a_u32", np.uint32, np.uint64), ("a_u64", np.uint64, np.uint32)])
def test_array_argument_types(bwtm, name, dtype, other):
    capi = bwtm.capi
    arg = getattr(capi, name)
    plain = getattr(capi, name.replace("a_", "p_"))
    assert arg.from_param(None) is None
    a = np.arange(8, dtype=dtype)
    assert ctypes.cast(arg.from_param(a), ctypes.c_void_p).value == a.ctypes.data
    assert ctypes.cast(arg.from_param(a.reshape(2, 4)), ctypes.c_void_p).value == a.ctypes.data
    p = a.ctypes.data_as(plain)
    assert arg.from_param(p) is p
    assert arg.from_param((plain._type_ * 3)()) is not None                  # what the plain pointer type takes: a ctypes array, a byref
    assert arg.from_param(ctypes.byref(plain._type_(0))) is not None
    for wrong in (a.astype(other), a[::2], a.reshape(2, 4).T, list(range(8)), 5, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int16))):
        with pytest.raises(TypeError):
            arg.from_param(wrong)
    assert plain is ctypes.POINTER(plain._type_)                             # the plain pointer types stay what raw calls are built with


def test_pack_texts(bwtm):
    pack = bwtm.capi.pack_texts
    for patterns, text, offsets in (([], [], [0]), ([(), (1, 2), ()], [1, 2], [0, 0, 2, 2]),
                                    ([np.array([5, 4], dtype=np.uint8), [3], np.zeros(0, dtype=np.int64)], [5, 4, 3], [0, 2, 3, 3])):
        t, o = pack(patterns)
        assert t.dtype == np.uint8 and o.dtype == np.uint64 and t.flags["C_CONTIGUOUS"] and o.flags["C_CONTIGUOUS"]
        assert t.tolist() == text and o.tolist() == offsets
