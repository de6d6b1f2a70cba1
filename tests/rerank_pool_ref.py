"""NumPy restatement of the pooled rerank (option "rerank_pool"): the exact score of every pooled id
and the order of the result.  The canonical sums are the oracle's ref_l2_distance_sqr / ref_dot (the eight-accumulator order of
src/math.rs), as tests/test_gpu_round2.py::test_optional_rerank_default_off takes them; the order is f32::total_cmp's key,
complemented for inner product, then the rank in the pool."""
import numpy as np

PAD_ID = np.uint64(0xFFFFFFFFFFFFFFFF)
NAN_BITS = np.uint32(0x7FC00000)


def total_key(x):
    """f32::total_cmp as an int32 key: ascending keys are ascending floats, -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN."""
    i = np.ascontiguousarray(x, np.float32).view(np.int32)
    return i ^ ((i >> 31).view(np.uint32) >> np.uint32(1)).view(np.int32)


def order_key(scores, metric):
    """the key the result is ordered by, ascending: smallest distance first (metric 0), largest dot product first (metric 1)"""
    k = total_key(scores)
    return ~k if metric == 1 else k


def exact_scores(query, raw, ids, metric):
    """canonical score of `query` with raw[id] for every id (f32); an id without a raw row scores the NaN 0x7fc00000"""
    import oracle
    L = oracle.lib()
    fn = L.ref_l2_distance_sqr if metric == 0 else L.ref_dot
    q = np.ascontiguousarray(query, np.float32)
    raw = np.ascontiguousarray(raw, np.float32)
    out = np.full(len(ids), NAN_BITS, np.uint32).view(np.float32)
    for r, i in enumerate(ids):
        if int(i) < raw.shape[0]:
            out[r] = fn(q.ctypes.data, raw[int(i)].ctypes.data, q.shape[0])
    return out


def order_pool(pool_ids, exact, count, metric, top_k):
    """One query.  pool_ids / exact: the pool by rank and its exact scores; count: its valid entries.
    Returns (ids[top_k] u64, score bits[top_k] u32, n): the first min(top_k, count) entries by (key, rank), padded."""
    c = int(count)
    key = order_key(np.asarray(exact, np.float32)[:c], metric).astype(np.int64)
    order = sorted(range(c), key=lambda r: (int(key[r]), r))[:top_k]
    ids = np.full(top_k, PAD_ID, np.uint64)
    bits = np.full(top_k, NAN_BITS, np.uint32)
    n = len(order)
    ids[:n] = np.asarray(pool_ids, np.uint64)[order]
    bits[:n] = np.asarray(exact, np.float32).view(np.uint32)[order]
    return ids, bits, n


def rerank_pool(queries, raw, pool_ids, pool_counts, metric, top_k):
    """The whole batch: (ids[nq, top_k] u64, score bits[nq, top_k] u32, counts[nq] u32) from the pools of a plain search."""
    nq = len(pool_counts)
    ids = np.empty((nq, top_k), np.uint64)
    bits = np.empty((nq, top_k), np.uint32)
    counts = np.empty(nq, np.uint32)
    for i in range(nq):
        c = int(pool_counts[i])
        ex = exact_scores(queries[i], raw, pool_ids[i, :c], metric)
        ids[i], bits[i], counts[i] = order_pool(pool_ids[i, :c], ex, c, metric, top_k)
    return ids, bits, counts
