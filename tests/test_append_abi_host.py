"""include/rbq_append.h without a GPU: the library exports the header's symbols, rbq.h includes the header, and the argument errors
that rbq_index_append finds before its first HIP call come back as RBQ_INVALID_CONFIG with their detail — those that can be
provoked without a live handle (null idx, null out)."""
import ctypes as C
import os

import numpy as np

import rabitq_rs_amd as rq
from c_header import c_functions
from conftest import ROOT
from rabitq_rs_amd import index as ix


def test_header_is_included_and_symbols_are_exported():
    hdr = open(os.path.join(ROOT, "include", "rbq.h")).read()
    assert '#include "rbq_append.h"' in hdr
    names = sorted(c_functions(open(os.path.join(ROOT, "include", "rbq_append.h")).read()))
    assert names == ["rbq_debug_append_carry_ns", "rbq_debug_append_passes", "rbq_index_append", "rbq_index_id_bound"]
    lib = ix.lib()
    for n in names:
        assert hasattr(lib, n), f"librbq.so does not export {n}"


def test_null_handle_and_null_out_are_invalid_config():
    lib = ix.lib()
    x = np.zeros((4, 16), np.float32)
    h = C.c_void_p(0xDEAD)  # must be cleared by the failing call
    rc = lib.rbq_index_append(None, x.ctypes.data, None, 4, 0, 0, 1.0, 0, 1, None, None, C.byref(h))
    assert rc == rq._abi.RBQ_INVALID_CONFIG and ix._detail() == "null index" and not h.value
    rc = lib.rbq_index_append(None, x.ctypes.data, None, 4, 0, 0, 1.0, 0, 1, None, None, None)
    assert rc == rq._abi.RBQ_INVALID_CONFIG and ix._detail() == "null out pointer"
    out = C.c_uint64(7)
    rc = lib.rbq_index_id_bound(None, C.byref(out))
    assert rc == rq._abi.RBQ_INVALID_CONFIG and "null" in ix._detail() and out.value == 7
    assert isinstance(lib.rbq_debug_append_passes(), int)
