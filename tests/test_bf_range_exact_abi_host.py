"""The C ABI of the exact brute-force range search (include/ext/rbq_bf_range.h) without a GPU: a call without
a handle is refused as rbq_bf_search_batch refuses it — first of all its checks, before any buffer or radius is looked at and
before the first HIP call — and a null handle has no raw rows."""
import numpy as np
import pytest

from rabitq_rs_amd import _abi, bruteforce as bfm, index as ix


@pytest.mark.parametrize("buffers", [True, False], ids=["buffers", "null_buffers"])
def test_null_index_is_refused_first_as_by_the_search(buffers):
    q, ids, sc, cnt = np.zeros((1, 16), np.float32), np.zeros((1, 4), np.uint64), np.zeros((1, 4), np.float32), np.zeros(1, np.uint32)
    qp, *out = (q.ctypes.data, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data) if buffers else (None, None, None, None)
    want = ix.lib().rbq_bf_search_batch(None, qp, 1, 16, 4, None, 0, *out), ix._detail()
    assert want == (_abi.RBQ_INVALID_CONFIG, "null index")
    for x, r in ((1.0, 2.0), (float("nan"), 2.0), (1.0, float("nan"))):
        assert (bfm.lib_ext().rbq_bf_range_exact_batch(None, qp, 1, 16, 4, x, r, None, 0, *out), ix._detail()) == want
    for dtype in (_abi.RAW_F32, 7):
        assert (bfm.lib_ext().rbq_bf_set_rerank_vectors(None, qp, 1, dtype), ix._detail()) == want
    assert bfm.lib_ext().rbq_bf_rerank_dtype(None) == -1
