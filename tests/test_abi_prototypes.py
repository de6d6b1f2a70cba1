"""The ctypes mirror of the C ABI (rabitq-rs_amd/_abi.py) held to the headers, without a GPU: every prototype of the two tables
against include/*.h and csrc/host/rbq_build.h, the five structure mirrors field for field, the constants against their #defines,
and, once the libraries are loaded, that every function object carries exactly its table entry.

One rule relates a header type to a ctypes type.  A scalar is its exact ctypes type (`void` as a return is None).  A returned
pointer is c_char_p for `const char*`, c_void_p for `void*`, POINTER(mirror or scalar) otherwise.  A pointer parameter is any
pointer-sized ctypes type, c_void_p, c_char_p (pointee char only) or POINTER(X), and where the table says POINTER(X), X is the
header's pointee.  The two function-pointer typedefs are passed as their CFUNCTYPE."""
import ctypes as C
import glob
import os

import pytest

from c_header import c_defines, c_fn_typedefs, c_functions, c_structs
from conftest import ROOT
from rabitq_rs_amd import _abi

INCLUDE = os.path.join(ROOT, "include")
BUILD_H = os.path.join(ROOT, "rabitq-rs_amd", "csrc", "host", "rbq_build.h")
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(INCLUDE, "*.h")))

SCALAR = {"u8": C.c_uint8, "u16": C.c_uint16, "u32": C.c_uint32, "u64": C.c_uint64, "c_int": C.c_int, "usize": C.c_size_t,
          "f32": C.c_float, "f64": C.c_double}
MIRROR = {"RbqHeader": _abi.Header, "RbqListView": _abi.ListView, "RbqDiag": _abi.Diag, "RbqBfView": _abi.BfView,
          "RbqMstgConfig": _abi.MstgConfig}
OPAQUE = ("c_void", "RbqIndex", "RbqBuilder", "RbqBfIndex", "RbqHclustered", "RbqBuilt", "RbqBfBuilt")
FN_TYPEDEF = {"RbqWriteFn": _abi.WRITE_FN, "RbqReadFn": _abi.READ_FN}


def read(path):
    with open(path) as f:
        return f.read()


def value_ctype(t):
    """the ctypes type of a header type that is held by value (a scalar, a struct, a function pointer) or pointed to"""
    if isinstance(t, tuple):
        inner = t[2]
        if inner in OPAQUE:
            return C.c_void_p
        if inner == "c_char":
            return C.c_char_p
        return C.POINTER(value_ctype(inner))
    return SCALAR.get(t) or MIRROR.get(t) or FN_TYPEDEF[t]


def check_return(name, got, t):
    want = None if t is None else value_ctype(t)
    assert got is want, f"{name}: returns {t}, declared {got}"


def check_param(name, pname, got, t):
    if not isinstance(t, tuple):
        assert got is value_ctype(t), f"{name}({pname}): {t} declared as {got}"
        return
    if got is C.c_void_p:
        return
    if got is C.c_char_p:
        assert t[2] == "c_char", f"{name}({pname}): c_char_p for {t}"
        return
    assert isinstance(got, type) and issubclass(got, C._Pointer), f"{name}({pname}): {t} declared as {got}, not a pointer type"
    assert got is value_ctype(t), f"{name}({pname}): POINTER({got._type_}) for {t}"


def check_table(group, functions, where):
    assert sorted(group) == sorted(functions), (where, sorted(set(group) ^ set(functions)))
    for name, (ret, params) in functions.items():
        restype, argtypes = group[name]
        check_return(name, restype, ret)
        assert len(argtypes) == len(params), f"{name}: {len(argtypes)} argtypes for {len(params)} parameters"
        for (pname, t), got in zip(params, argtypes):
            check_param(name, pname, got, t)


def test_the_librbq_table_has_one_group_per_public_header():
    assert sorted(_abi.LIBRBQ_BY_HEADER) == HEADERS and len(HEADERS) == 10
    assert sum(len(g) for g in _abi.LIBRBQ_BY_HEADER.values()) == len(_abi.LIBRBQ) == 109  # no name in two groups


@pytest.mark.parametrize("header", HEADERS)
def test_librbq_prototypes_match_their_header(header):
    check_table(_abi.LIBRBQ_BY_HEADER[header], c_functions(read(os.path.join(INCLUDE, header))), header)


def test_builder_prototypes_match_rbq_build_h():
    functions = c_functions(read(BUILD_H))
    assert len(functions) == 34
    check_table(_abi.LIBRBQ_BUILD, functions, "rbq_build.h")
    for name, proto in _abi.HCLUSTERED.items():  # listed once, part of both tables
        assert _abi.LIBRBQ_BUILD[name] is proto and _abi.LIBRBQ[name] is proto


def test_callback_types_match_their_typedefs():
    typedefs = c_fn_typedefs(read(os.path.join(INCLUDE, "rbq_persist.h")))
    assert sorted(typedefs) == ["rbq_read_fn", "rbq_write_fn"]
    for name, fn in (("rbq_write_fn", _abi.WRITE_FN), ("rbq_read_fn", _abi.READ_FN)):
        ret, params = typedefs[name]
        check_return(name, fn._restype_, ret)
        assert len(fn._argtypes_) == len(params)
        for (pname, t), got in zip(params, fn._argtypes_):
            check_param(name, pname, got, t)


def test_structure_mirrors_match_their_typedefs_field_for_field():
    structs = {}
    for header in HEADERS:
        structs.update(c_structs(read(os.path.join(INCLUDE, header))))
    assert sorted(structs) == sorted(MIRROR)
    for name, mirror in MIRROR.items():
        assert [f for f, _ in mirror._fields_] == [f for f, _ in structs[name]], name
        for (field, got), (_, t) in zip(mirror._fields_, structs[name]):
            assert got is value_ctype(t), (name, field, got, t)
    assert [C.sizeof(MIRROR[n]) for n in ("RbqHeader", "RbqListView", "RbqDiag", "RbqBfView", "RbqMstgConfig")] == [48, 64, 24, 96, 88]
    assert _abi.MSTG_CONFIG_FIELDS == tuple(f for f, _ in _abi.MstgConfig._fields_)
    assert tuple(f for f, _ in _abi.BfView._fields_[4:]) == _abi.BF_FACTORS


def test_constants_match_their_defines():
    defines = {}
    for header in HEADERS:
        defines.update(c_defines(read(os.path.join(INCLUDE, header))))
    errors = ("OK", "DIMENSION_MISMATCH", "INVALID_CONFIG", "EMPTY_INDEX", "IO", "INVALID_PERSISTENCE", "DEVICE")
    mirrored = {"RBQ_" + n: getattr(_abi, "RBQ_" + n) for n in errors}
    for prefix, names in (("METRIC", ("L2", "IP")), ("ROTATOR", ("MATRIX", "FHT_KAC", "NONE")),
                          ("NUMERIC", ("NATIVE_AVX512", "NATIVE_AVX2", "PORTABLE")), ("RESCALE", ("CONST", "OPTIMAL"))):
        mirrored.update({f"RBQ_{prefix}_{n}": getattr(_abi, f"{prefix}_{n}") for n in names})
        assert sorted(d for d in defines if d.startswith(f"RBQ_{prefix}_")) == sorted(f"RBQ_{prefix}_{n}" for n in names)  # none left out
    mirrored.update(RBQ_BATCH=_abi.BATCH, RBQ_MSTG_REFINE_POOL_MAX=_abi.MSTG_REFINE_POOL_MAX)
    assert len(mirrored) == 19
    for name, value in mirrored.items():
        assert defines[name] == value, name
    assert sorted(_abi.NUMERIC_VARIANTS.values()) == [0, 1, 2] and sorted(_abi.RESCALE_MODES.values()) == [0, 1]


def test_loaded_libraries_carry_exactly_their_tables():
    from rabitq_rs_amd import bruteforce, builder, index
    assert bruteforce.lib() is index.lib()
    for L, table in ((index.lib(), _abi.LIBRBQ), (builder.lib(), _abi.LIBRBQ_BUILD)):
        bound = {n: f for n, f in vars(L).items() if isinstance(f, C._CFuncPtr)}
        assert set(bound) >= set(table), sorted(set(table) - set(bound))  # every table name resolved as a symbol at lib()
        for name, fn in bound.items():
            assert name in table, f"{name} is called without a declaration"
            restype, argtypes = table[name]
            assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
