"""The C ABI of the MSTG range search (include/ext/rbq_mstg_range.h, rbq_mstg_range_batch*) without a GPU: the binding's table of
its own (_abi.LIBRBQ_EXT) is held to the header by the rule test_abi_prototypes holds the main table by, the loaded entries carry
exactly that table, the limit is the header's, and a call without a handle is refused as rbq_mstg_search_batch refuses it — first
of all its checks, before any buffer is looked at and before the first HIP call."""
import ctypes as C
import os

import numpy as np
import pytest

from c_header import c_defines, c_functions
from conftest import ROOT
from rabitq_rs_amd import _abi, index as ix
from test_abi_prototypes import check_table

NAME = "ext/rbq_mstg_range.h"
HEADER = open(os.path.join(ROOT, "include", NAME)).read()


def test_ext_table_matches_its_header_and_the_loaded_entries():
    assert sorted(_abi.LIBRBQ_EXT_BY_HEADER) == [NAME] and not set(_abi.LIBRBQ_EXT) & set(_abi.LIBRBQ)
    declared = c_functions(HEADER)
    check_table(_abi.LIBRBQ_EXT_BY_HEADER[NAME], declared, NAME)
    bound = {n: f for n, f in vars(ix.lib_ext()).items() if isinstance(f, C._CFuncPtr)}
    assert sorted(bound) == sorted(_abi.LIBRBQ_EXT) == ["rbq_mstg_range_batch", "rbq_mstg_range_batch_device"]
    search = c_functions(open(os.path.join(ROOT, "include", "rbq_mstg.h")).read())
    for name, fn in bound.items():
        assert (fn.restype, list(fn.argtypes)) == (_abi.LIBRBQ_EXT[name][0], list(_abi.LIBRBQ_EXT[name][1]))
        want = [p for p, _ in search[name.replace("range", "search")][1]]  # the search's arguments, top_k renamed, two more
        want[want.index("top_k")] = "capacity"
        at = want.index("pruning_epsilon") + 1
        assert [p for p, _ in declared[name][1]] == want[:at] + ["radius", "distinct"] + want[at:]
    assert c_defines(HEADER)["RBQ_MSTG_RANGE_DISTINCT_MAX"] == _abi.MSTG_RANGE_DISTINCT_MAX == 4096


@pytest.mark.parametrize("buffers", [True, False], ids=["buffers", "null_buffers"])
def test_null_index_is_refused_first_as_by_the_search(buffers):
    L, X = ix.lib(), ix.lib_ext()
    q, ids, sc, cnt = np.zeros((1, 16), np.float32), np.zeros((1, 4), np.uint64), np.zeros((1, 4), np.float32), np.zeros(1, np.uint32)
    qp, *out = (q.ctypes.data, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data) if buffers else (None, None, None, None)
    want = L.rbq_mstg_search_batch(None, qp, 1, 16, 4, 6, 0.6, *out, None, None), ix._detail()
    assert want == (_abi.RBQ_INVALID_CONFIG, "null index")
    assert (X.rbq_mstg_range_batch(None, qp, 1, 16, 4, 6, 0.6, 1.0, 1, *out, None, None), ix._detail()) == want
    assert (X.rbq_mstg_range_batch_device(None, qp, 1, 16, 4, 6, 0.6, 1.0, 0, *out, None, None, None), ix._detail()) == want
