"""The C ABI of the brute-force range search (include/ext/rbq_bf_range.h) without a GPU: the binding's table of its own
(_abi.LIBRBQ_BF_EXT) is held to the header by the rule test_abi_prototypes holds the main table by, the entries loaded on
bruteforce.lib_ext() carry exactly that table, and a call without a handle is refused as rbq_bf_search_batch refuses it — first of
all its checks, before any buffer is looked at and before the first HIP call."""
import ctypes as C
import os

import numpy as np
import pytest

from c_header import c_functions
from conftest import ROOT
from rabitq_rs_amd import _abi, bruteforce as bfm, index as ix
from test_abi_prototypes import check_table

NAME = "ext/rbq_bf_range.h"


def test_bf_ext_table_matches_its_header_and_the_loaded_entries():
    assert sorted(_abi.LIBRBQ_BF_EXT_BY_HEADER) == [NAME]
    assert not set(_abi.LIBRBQ_BF_EXT) & (set(_abi.LIBRBQ) | set(_abi.LIBRBQ_EXT))
    check_table(_abi.LIBRBQ_BF_EXT_BY_HEADER[NAME], c_functions(open(os.path.join(ROOT, "include", NAME)).read()), NAME)
    bound = {n: f for n, f in vars(bfm.lib_ext()).items() if isinstance(f, C._CFuncPtr)}
    assert sorted(bound) == sorted(_abi.LIBRBQ_BF_EXT) and "rbq_bf_range_batch" in bound
    for name, fn in bound.items():
        assert (fn.restype, list(fn.argtypes)) == (_abi.LIBRBQ_BF_EXT[name][0], list(_abi.LIBRBQ_BF_EXT[name][1]))


@pytest.mark.parametrize("buffers", [True, False], ids=["buffers", "null_buffers"])
def test_null_index_is_refused_first_as_by_the_search(buffers):
    q, ids, sc, cnt = np.zeros((1, 16), np.float32), np.zeros((1, 4), np.uint64), np.zeros((1, 4), np.float32), np.zeros(1, np.uint32)
    qp, *out = (q.ctypes.data, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data) if buffers else (None, None, None, None)
    want = ix.lib().rbq_bf_search_batch(None, qp, 1, 16, 4, None, 0, *out), ix._detail()
    assert want == (_abi.RBQ_INVALID_CONFIG, "null index")
    assert (bfm.lib_ext().rbq_bf_range_batch(None, qp, 1, 16, 4, 1.0, None, 0, *out), ix._detail()) == want
    assert (bfm.lib_ext().rbq_bf_range_batch(None, qp, 1, 16, 4, float("nan"), None, 0, *out), ix._detail()) == want
