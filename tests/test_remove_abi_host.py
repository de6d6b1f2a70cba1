"""include/rbq_remove.h without a GPU: the library exports the header's symbols, rbq.h includes the header, and the argument errors
that rbq_index_remove_ids finds before its first HIP call come back as RBQ_INVALID_CONFIG with their detail, in the documented
order — those that can be provoked without a live handle (null out, then null idx; the later ones need a handle and are in
tests/test_gpu_remove.py)."""
import ctypes as C
import os

import numpy as np

import rabitq_rs_amd as rq
from c_header import c_functions
from conftest import ROOT
from rabitq_rs_amd import index as ix


def test_header_is_included_and_symbols_are_exported():
    hdr = open(os.path.join(ROOT, "include", "rbq.h")).read()
    assert '#include "rbq_remove.h"' in hdr and hdr.index('#include "rbq_append.h"') < hdr.index('#include "rbq_remove.h"')
    names = sorted(c_functions(open(os.path.join(ROOT, "include", "rbq_remove.h")).read()))
    assert names == ["rbq_debug_remove_gather_ns", "rbq_index_remove_ids"]
    lib = ix.lib()
    for n in names:
        assert hasattr(lib, n), f"librbq.so does not export {n}"
    lib.rbq_abi_version.restype = C.c_uint32
    assert lib.rbq_abi_version() & 0xFFFF == 2  # the minor version stays 2: a caller finds the entry points by their symbols


def test_null_out_then_null_handle_are_invalid_config():
    lib = ix.lib()
    ids = np.arange(4, dtype=np.uint64)
    removed = C.c_uint64(7)
    # null out comes first: nothing else is looked at
    rc = lib.rbq_index_remove_ids(None, None, 0, 99, None, C.byref(removed), None)
    assert rc == rq._abi.RBQ_INVALID_CONFIG and ix._detail() == "null out pointer" and removed.value == 7
    # then the null handle, before null ids, n_ids == 0 and the device list; *out is cleared by the failing call
    for args in ((ids.ctypes.data, 4, 1, None), (None, 4, 1, None), (ids.ctypes.data, 0, 1, None), (ids.ctypes.data, 4, 99, None)):
        h = C.c_void_p(0xDEAD)
        rc = lib.rbq_index_remove_ids(None, *args, C.byref(removed), C.byref(h))
        assert rc == rq._abi.RBQ_INVALID_CONFIG and ix._detail() == "null index" and not h.value and removed.value == 7
    assert isinstance(lib.rbq_debug_remove_gather_ns(), int)
