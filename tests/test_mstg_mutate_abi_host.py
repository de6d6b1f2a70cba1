"""include/rbq_mstg_mutate.h without a GPU: rbq_mstg.h includes the header, the library exports its symbols, the prototypes match
the ctypes declarations of _abi.py argument for argument, rbq_abi_version() is still 2.2, and the argument errors both calls find
before their first HIP call come back as RBQ_INVALID_CONFIG with their detail — those that can be provoked without a live handle."""
import ctypes as C
import os
import re

import numpy as np

import rabitq_rs_amd as rq
from conftest import ROOT
from rabitq_rs_amd import _abi
from rabitq_rs_amd import index as ix

CTYPE = {"int": C.c_int, "float": C.c_float, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "void": None}


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rbq_mstg_mutate.h")).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int|uint64_t)\s+(rbq_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        types = []
        for a in [a.strip() for a in args.split(",")]:
            if a == "void":
                continue
            base = re.sub(r"\bconst\b", "", a)
            stars = base.count("*")
            word = re.findall(r"[A-Za-z_][A-Za-z0-9_]*", base)[0]
            types.append((word, stars))
        out[name] = (ret, types)
    return out


def _ctype_of(word, stars):
    if stars == 0:
        return CTYPE[word]
    if stars == 2 and word == "rbq_index":
        return C.POINTER(C.c_void_p)  # rbq_index** out
    return C.c_void_p


def test_prototypes_match_the_ctypes_declarations():
    protos = _prototypes()
    assert sorted(protos) == sorted(_abi.MSTG_MUTATE_PROTOTYPES) == ["rbq_debug_mstg_append_passes", "rbq_mstg_append",
                                                                      "rbq_mstg_remove_ids"]
    lib = ix.lib()
    for name, (ret, types) in protos.items():
        res, args = _abi.MSTG_MUTATE_PROTOTYPES[name]
        assert res is CTYPE[ret], name
        assert len(args) == len(types), name
        for i, ((word, stars), got) in enumerate(zip(types, args)):
            want = _ctype_of(word, stars)
            if name == "rbq_mstg_remove_ids" and word == "uint64_t" and stars == 1 and i == 3:
                want = C.POINTER(C.c_uint64)  # out_removed: written through, declared as a typed pointer
            assert got is want or (got == want), (name, i, word, stars, got)
        fn = getattr(lib, name)  # librbq.so exports it and index.lib() applied the declaration
        assert fn.restype is res and list(fn.argtypes or []) == list(args)


def test_header_is_included_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "rbq_mstg.h")).read()
    assert '#include "rbq_mstg_mutate.h"' in hdr
    assert ix.lib().rbq_abi_version() == (2 << 16) | 2


def test_null_handle_and_null_out_are_invalid_config():
    lib = ix.lib()
    x = np.zeros((4, 16), np.float32)
    ids = np.arange(3, dtype=np.uint64)
    h = C.c_void_p(0xDEAD)  # must be cleared by the failing call
    rc = lib.rbq_mstg_append(None, x.ctypes.data, 4, 0, 0.15, 8, 0, None, None, C.byref(h))
    assert rc == rq._abi.RBQ_INVALID_CONFIG and ix._detail() == "null index" and not h.value
    rc = lib.rbq_mstg_append(None, x.ctypes.data, 4, 0, 0.15, 8, 0, None, None, None)
    assert rc == rq._abi.RBQ_INVALID_CONFIG and ix._detail() == "null out pointer"
    h = C.c_void_p(0xDEAD)
    removed = C.c_uint64(7)
    rc = lib.rbq_mstg_remove_ids(None, ids.ctypes.data, 3, C.byref(removed), C.byref(h))
    assert rc == rq._abi.RBQ_INVALID_CONFIG and ix._detail() == "null index" and not h.value and removed.value == 7
    rc = lib.rbq_mstg_remove_ids(None, ids.ctypes.data, 3, None, None)
    assert rc == rq._abi.RBQ_INVALID_CONFIG and ix._detail() == "null out pointer"
    assert isinstance(lib.rbq_debug_mstg_append_passes(), int)
    assert callable(rq.append_postings) and callable(rq.remove_postings)
