"""The C ABI of the ranked exact brute-force top-k (rbq_bf_search_exact_ranked_batch) without a GPU: a call
without a handle is refused as rbq_bf_search_batch refuses it — first of all its checks, whatever the buffers, top_k and pool are."""
import numpy as np
import pytest

from rabitq_rs_amd import _abi, bruteforce as bfm, index as ix


@pytest.mark.parametrize("buffers", [True, False], ids=["buffers", "null_buffers"])
@pytest.mark.parametrize("top_k,pool", [(4, 4), (0, 4), (4, 5000), (0, 5000)])
def test_null_index_is_refused_first_as_by_the_search(buffers, top_k, pool):
    q, ids, sc, cnt = np.zeros((1, 16), np.float32), np.zeros((1, 4), np.uint64), np.zeros((1, 4), np.float32), np.zeros(1, np.uint32)
    qp, *out = (q.ctypes.data, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data) if buffers else (None, None, None, None)
    want = ix.lib().rbq_bf_search_batch(None, qp, 1, 16, 4, None, 0, *out), ix._detail()
    assert want == (_abi.RBQ_INVALID_CONFIG, "null index")
    assert (bfm.lib_ext().rbq_bf_search_exact_ranked_batch(None, qp, 1, 16, top_k, pool, None, 0, *out), ix._detail()) == want
