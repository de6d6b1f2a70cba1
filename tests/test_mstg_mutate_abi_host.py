"""include/rbq_mstg_mutate.h without a GPU: rbq_mstg.h includes the header, rbq_abi_version() is still 2.2, and the argument errors
both calls find before their first HIP call come back as RBQ_INVALID_CONFIG with their detail — those that can be provoked without
a live handle.  (That the library exports the header's symbols and that the prototypes match the ctypes declarations of _abi.py
argument for argument is test_abi_prototypes.py's, for this header as for every other.)"""
import ctypes as C
import os

import numpy as np

import rabitq_rs_amd as rq
from conftest import ROOT
from rabitq_rs_amd import index as ix


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
