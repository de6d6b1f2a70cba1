"""include/rbq_bf_mutate.h without a GPU: the library exports the header's entry points with the documented prototypes, rbq_bf.h
includes the header, the minor ABI version stays 2, the argument errors that rbq_bf_append / rbq_bf_remove_ids /
rbq_bf_fetch_embeddings* find before their first HIP call and that can be provoked without a live handle (null out, then null
idx) come back as RBQ_INVALID_CONFIG with their detail and with *out cleared, and BruteForceRabitqIndex.add on an object that does
not remember its rescale mode raises before any call.  The errors that need a handle are in tests/test_gpu_bf_mutate.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rabitq_rs_amd as rq
from c_header import c_functions, strip_c_comments
from conftest import ROOT
from rabitq_rs_amd import bruteforce as bfm
from rabitq_rs_amd import index as ix

INVALID = rq._abi.RBQ_INVALID_CONFIG

PROTOTYPES = [
    r"int rbq_bf_append\(const rbq_bf_index\* idx, const float\* vectors, uint64_t count, int rescale, float t_const,\s*"
    r"uint64_t max_chunk_rows, rbq_bf_index\*\* out\);",
    r"int rbq_bf_remove_ids\(const rbq_bf_index\* idx, const uint64_t\* ids, uint64_t n_ids, uint64_t\* out_removed,\s*"
    r"rbq_bf_index\*\* out\);",
    r"int rbq_bf_fetch_embeddings\(const rbq_bf_index\* idx, const uint64_t\* ids, uint64_t n, float\* out, uint8_t\* found\);",
    r"int rbq_bf_fetch_embeddings_device\(const rbq_bf_index\* idx, const uint64_t\* d_ids, uint64_t n, float\* d_out,\s*"
    r"uint8_t\* d_found, void\* hip_stream\);",
]


def test_header_is_included_and_symbols_are_exported_and_declared():
    assert '#include "rbq_bf_mutate.h"' in open(os.path.join(ROOT, "include", "rbq_bf.h")).read()
    text = open(os.path.join(ROOT, "include", "rbq_bf_mutate.h")).read()
    src = strip_c_comments(text)
    for proto in PROTOTYPES:
        assert re.search(proto, src), proto
    names = sorted(c_functions(text))
    assert names == ["rbq_bf_append", "rbq_bf_debug_append_carry_ns", "rbq_bf_debug_remove_gather_ns", "rbq_bf_fetch_embeddings",
                     "rbq_bf_fetch_embeddings_device", "rbq_bf_remove_ids"]
    lib = bfm.lib()
    for n in names:
        assert hasattr(lib, n), f"librbq.so does not export {n}"
    assert "RENUMBERED" in text and "IndexFlat::remove_ids" in text  # the header says plainly that ids are positions
    lib.rbq_abi_version.restype = C.c_uint32
    assert lib.rbq_abi_version() & 0xFFFF == 2  # the minor version stays 2: a caller finds the entry points by their symbols
    assert isinstance(lib.rbq_bf_debug_append_carry_ns(), int) and isinstance(lib.rbq_bf_debug_remove_gather_ns(), int)


def test_append_null_out_then_null_handle():
    lib = bfm.lib()
    x = np.zeros((2, 64), np.float32)
    rc = lib.rbq_bf_append(None, None, 0, 99, 0.0, 0, None)  # null out comes first: nothing else is looked at
    assert rc == INVALID and ix._detail() == "null output"
    # then the null handle, before null vectors, count == 0 and the rescale mode; *out is cleared by the failing call
    for vec, count, rescale in ((x.ctypes.data, 2, 0), (None, 2, 0), (x.ctypes.data, 0, 0), (x.ctypes.data, 2, 99)):
        h = C.c_void_p(0xDEAD)
        rc = lib.rbq_bf_append(None, vec, count, rescale, 1.5, 0, C.byref(h))
        assert rc == INVALID and ix._detail() == "null index" and not h.value


def test_remove_null_out_then_null_handle():
    lib = bfm.lib()
    ids = np.arange(4, dtype=np.uint64)
    removed = C.c_uint64(7)
    rc = lib.rbq_bf_remove_ids(None, None, 0, C.byref(removed), None)
    assert rc == INVALID and ix._detail() == "null output" and removed.value == 7
    for p, n in ((ids.ctypes.data, 4), (None, 4), (ids.ctypes.data, 0)):
        h = C.c_void_p(0xDEAD)
        rc = lib.rbq_bf_remove_ids(None, p, n, C.byref(removed), C.byref(h))
        assert rc == INVALID and ix._detail() == "null index" and not h.value and removed.value == 7


def test_fetch_null_handle():
    lib = bfm.lib()
    ids = np.arange(4, dtype=np.uint64)
    out, found = np.zeros((4, 64), np.float32), np.zeros(4, np.uint8)
    rc = lib.rbq_bf_fetch_embeddings(None, ids.ctypes.data, 4, out.ctypes.data, found.ctypes.data)
    assert rc == INVALID and ix._detail() == "null index"
    rc = lib.rbq_bf_fetch_embeddings_device(None, ids.ctypes.data, 4, out.ctypes.data, found.ctypes.data, None)
    assert rc == INVALID and ix._detail() == "null index"


def test_python_add_needs_to_know_the_rescale_mode():
    """an object from load_from_* or from_built wraps a handle that does not remember what it was encoded with: add() says so
    before it calls the library (the handle here is never touched)"""
    idx = rq.BruteForceRabitqIndex(None)
    with pytest.raises(rq.RabitqError, match="does not know what it was encoded with") as e:
        idx.add(np.zeros((2, 64), np.float32))
    assert e.value.kind == "InvalidConfig"


def test_python_remove_of_nothing_makes_no_call():
    idx = rq.BruteForceRabitqIndex(None)
    assert idx.remove_ids([]) == 0 and idx.remove_ids(np.zeros(0, np.uint64)) == 0
