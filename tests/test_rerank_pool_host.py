"""The pooled rerank's restatement (tests/rerank_pool_ref.py) against hand-written cases: the order of the result is
f32::total_cmp's, complemented for inner product, then the rank in the pool.  No GPU."""
import numpy as np

from rerank_pool_ref import NAN_BITS, PAD_ID, order_key, order_pool, total_key


def _f(*bits):
    return np.array(bits, np.uint32).view(np.float32)


NAN = _f(0x7FC00000)[0]


def test_total_key_is_total_cmp():
    xs = _f(0xFFC00000, 0xFF800000, 0xBF800000, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x3F800000, 0x7F800000, 0x7FC00000)
    k = total_key(xs)  # -NaN, -inf, -1, -denormal, -0.0, +0.0, +denormal, 1, +inf, +NaN
    assert (np.diff(k.astype(np.int64)) > 0).all()


def test_negative_zero_before_positive_zero():
    ex = np.array([0.0, -0.0, 1.0], np.float32)
    ids, bits, n = order_pool([10, 11, 12], ex, 3, 0, 3)
    assert n == 3 and ids.tolist() == [11, 10, 12]
    assert bits.tolist() == [0x80000000, 0x00000000, 0x3F800000]
    ids, bits, n = order_pool([10, 11, 12], ex, 3, 1, 3)  # inner product: descending, so +0.0 comes before -0.0
    assert ids.tolist() == [12, 10, 11] and bits.tolist() == [0x3F800000, 0x00000000, 0x80000000]


def test_nan_last_for_l2_first_for_inner_product():
    ex = np.array([2.0, NAN, np.inf, -1.0], np.float32)
    ids, bits, n = order_pool([5, 6, 7, 8], ex, 4, 0, 4)
    assert ids.tolist() == [8, 5, 7, 6] and bits[3] == NAN_BITS
    ids, bits, n = order_pool([5, 6, 7, 8], ex, 4, 1, 4)
    assert ids.tolist() == [6, 7, 5, 8] and bits[0] == NAN_BITS
    assert order_key(np.array([NAN], np.float32), 1)[0] < order_key(np.array([np.inf], np.float32), 1)[0]


def test_equal_scores_keep_rank_order():
    ex = np.array([3.0, 1.0, 3.0, 1.0, 3.0], np.float32)
    for metric, want in ((0, [21, 23, 20, 22, 24]), (1, [20, 22, 24, 21, 23])):
        ids, _, n = order_pool([20, 21, 22, 23, 24], ex, 5, metric, 5)
        assert n == 5 and ids.tolist() == want
    ids, _, n = order_pool([20, 21, 22, 23, 24], ex, 5, 0, 3)  # the cut falls inside a run of equal scores
    assert n == 3 and ids.tolist() == [21, 23, 20]


def test_count_below_top_k_is_padded():
    ex = np.array([4.0, 2.0, 9.0, 9.0], np.float32)  # (entries past the count are not part of the pool)
    ids, bits, n = order_pool([1, 2, 3, 4], ex, 2, 0, 5)
    assert n == 2 and ids.tolist() == [2, 1] + [int(PAD_ID)] * 3
    assert bits.tolist() == [0x40000000, 0x40800000] + [int(NAN_BITS)] * 3


def test_empty_pool():
    ids, bits, n = order_pool(np.empty(0, np.uint64), np.empty(0, np.float32), 0, 1, 4)
    assert n == 0 and (ids == PAD_ID).all() and (bits == NAN_BITS).all()
