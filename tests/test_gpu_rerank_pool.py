"""The pooled rerank (option "rerank_pool"; k_rerank_pool.hip): with raw vectors attached and a pool above
top_k a search takes `pool` candidates by the estimate, scores them exactly and returns the best top_k.  Held against the
existing rerank kernel at top_k := pool (up to its limit of 1024), against the NumPy restatement (tests/rerank_pool_ref.py)
beyond it, and against the exact top_k over every row when the pool holds the whole index."""
import ctypes as C
import functools

import numpy as np
import pytest

import rabitq_rs_amd as rq
from conftest import build_index, make_dataset
from rabitq_rs_amd import index as rq_index
from rerank_pool_ref import NAN_BITS, PAD_ID, exact_scores, order_key, rerank_pool

pytestmark = pytest.mark.gpu

_OPEN = []


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    for idx in _OPEN:
        idx.close()
    _OPEN.clear()
    _case.cache_clear()


@functools.lru_cache(maxsize=None)
def _case(dim, metric, n=3000, nlist=12, bits=7, seed=2700):
    """(data, built, index with the raw vectors attached); one per shape for the whole module"""
    data, built = build_index(n=n, dim=dim, nlist=nlist, total_bits=bits, metric=metric, normalize=(metric == 1 and dim > 1),
                              seed=seed + dim)
    idx = rq.IvfRabitqIndex.from_built(built)
    idx.set_rerank_vectors(data)
    _OPEN.append(idx)
    return data, built, idx


def _queries(nq, dim, metric, seed=2790):
    return make_dataset(nq, dim, 3, seed + dim, normalize=(metric == 1 and dim > 1))


def _search(idx, q, top_k, nprobe, rerank, pool, **kw):
    """one host call with the rerank and the pool set as given; (ids, score bits, counts, diag)"""
    idx.set_option("rerank", rerank)
    idx.set_rerank_pool(pool)
    try:
        ids, sc, cnt, diag = idx.batch_search_raw(q, rq.SearchParams(top_k, nprobe), **kw)
    finally:
        idx.set_rerank_pool(0)
        idx.set_option("rerank", 1)
    return ids, sc.view(np.uint32), cnt, diag


def _assert_same(got, want, what=""):
    assert np.array_equal(got[2], want[2]), what
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what


def _restated(idx, data, q, top_k, nprobe, pool, metric, raw=None, **kw):
    """the restatement over the pool of the plain search at top_k := pool"""
    pid, _, pcnt, diag = _search(idx, q, pool, nprobe, 0, 0, **kw)
    ids, bits, cnt = rerank_pool(q, data if raw is None else raw, pid, pcnt, metric, top_k)
    return (ids, bits, cnt, diag), pcnt


# ---- against the existing kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_k,pool", [(1, 2), (10, 63), (10, 64), (10, 65), (10, 256), (10, 257), (100, 1024)])
@pytest.mark.parametrize("dim", [1, 7, 8, 20, 96, 100, 2047])
@pytest.mark.parametrize("metric", [0, 1])
def test_head_of_the_existing_rerank_at_pool(metric, dim, top_k, pool):
    """pool <= 1024: the result is the first top_k entries of today's reranked result at top_k := pool, bit for bit (256 | 257: the
    inner search's top-k leaves the registers for the LDS heap; dim 1, 7: no main chunk; 20, 100: a tail after chunks and a row
    that starts off a 16-byte boundary; 100: FHT-padded; 2047: the widest query row)."""
    data, built, idx = _case(dim, metric)
    q = _queries(12, dim, metric)
    got = _search(idx, q, top_k, 6, 1, pool)
    rid, rsc, rcnt, _ = _search(idx, q, pool, 6, 1, 0)
    assert rcnt.max() > top_k  # (the pool holds more than the answer)
    want_cnt = np.minimum(rcnt, top_k).astype(np.uint32)
    _assert_same(got, (rid[:, :top_k], rsc[:, :top_k], want_cnt))


# ---- against the restatement beyond the old limit ---------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("top_k,pool,nprobe", [(10, 1025, 12), (10, 4096, 12), (3500, 4096, 12)])
def test_restatement_beyond_1024(metric, top_k, pool, nprobe):
    """pools the old kernel does not take: 1025 (full), 4096 over an index of 3000 vectors (the pool ends at c = 3000 < pool),
    and the same under top_k = 3500 (c < top_k: the answer ends at c and is padded after; a pooled call is not bound to
    top_k <= 1024, its inner search runs with the rerank off)."""
    data, built, idx = _case(100, metric)
    q = _queries(5, 100, metric)
    want, pcnt = _restated(idx, data, q, top_k, nprobe, pool, metric)
    assert (pcnt == min(pool, 3000)).all()
    got = _search(idx, q, top_k, nprobe, 1, pool)
    _assert_same(got, want)
    pad = np.arange(top_k)[None, :] >= got[2][:, None]
    assert (got[0][pad] == PAD_ID).all() and (got[1][pad] == NAN_BITS).all()


# ---- the pool holds the whole index: the exact top_k ------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_exhaustive_pool_gives_the_exact_top_k(metric):
    """nprobe = nlist and pool >= n: the heap never fills, every vector is pooled, and the answer is the exact top_k over ALL
    rows by the canonical score — which the unpooled rerank, bound to the ids the estimate returned, does not reach."""
    n, top_k = 2000, 10
    data, built, idx = _case(96, metric, n=n, nlist=8, bits=1, seed=2710)
    q = _queries(6, 96, metric)
    assert (_search(idx, q, 2048, 8, 0, 0)[2] == n).all()  # (every vector is in the pool)
    got = _search(idx, q, top_k, 8, 1, 2048)
    assert (got[2] == top_k).all()
    for i in range(q.shape[0]):
        ex = exact_scores(q[i], data, np.arange(n), metric)
        order = np.argsort(order_key(ex, metric).astype(np.int64), kind="stable")[:top_k + 1]
        bits = ex.view(np.uint32)[order]
        assert np.array_equal(got[1][i], bits[:top_k])
        # an id is determined wherever its score differs from both neighbours' (the next one past the cut included)
        lone = np.ones(top_k, bool)
        same = bits[1:] == bits[:-1]
        lone[:top_k] &= ~same[:top_k]
        lone[1:] &= ~same[:top_k - 1]
        assert np.array_equal(got[0][i][lone], order[:top_k].astype(np.uint64)[lone])
        assert len(set(got[0][i].tolist())) == top_k
        assert np.array_equal(ex.view(np.uint32)[got[0][i].astype(np.int64)], got[1][i])  # (inside a run of equal scores: one of its ids)


# ---- edges ------------------------------------------------------------------------------------------------------------
def _filter_words(allowed, nbits):
    words = np.zeros((nbits + 31) // 32, np.uint32)
    allowed = np.asarray(allowed, np.int64)
    np.bitwise_or.at(words, allowed >> 5, (np.uint32(1) << (allowed & 31).astype(np.uint32)))
    return words


@pytest.mark.parametrize("metric", [0, 1])
def test_filters(metric):
    data, built, idx = _case(20, metric)
    q = _queries(7, 20, metric)
    none = _search(idx, q, 10, 12, 1, 64, filter_words=_filter_words([], 3000), filter_nbits=3000)
    assert (none[2] == 0).all() and (none[0] == PAD_ID).all() and (none[1] == NAN_BITS).all()
    few = dict(filter_words=_filter_words([3, 700, 701, 1500, 2999], 3000), filter_nbits=3000)
    want, pcnt = _restated(idx, data, q, 10, 12, 64, metric, **few)
    assert (pcnt == 5).all()
    got = _search(idx, q, 10, 12, 1, 64, **few)
    _assert_same(got, want)
    assert (got[0][:, 5:] == PAD_ID).all() and (got[1][:, 5:] == NAN_BITS).all()
    many = dict(filter_words=_filter_words(np.arange(0, 3000, 3), 3000), filter_nbits=3000)
    want, _ = _restated(idx, data, q, 10, 12, 64, metric, **many)
    _assert_same(_search(idx, q, 10, 12, 1, 64, **many), want)


@pytest.mark.parametrize("metric", [0, 1])
def test_ids_without_a_raw_row_score_nan(metric):
    """vectors attached for the first 1500 rows only: an id past them scores the NaN 0x7fc00000, which the key puts last for L2
    and first for inner product"""
    data, built, _ = _case(20, metric)
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        idx.set_rerank_vectors(data[:1500])
        q = _queries(9, 20, metric)
        want, _ = _restated(idx, data, q, 290, 12, 300, metric, raw=data[:1500])
        got = _search(idx, q, 290, 12, 1, 300)
        _assert_same(got, want)
        assert (got[2] == 290).all()
        nan = got[1] == NAN_BITS
        assert nan.any() and (~nan).any() and (got[0][nan] >= 1500).all() and (got[0][~nan] < 1500).all()
        step = np.diff(nan.astype(np.int8), axis=1)  # one block of NaN entries per row: at the end for L2, at the start for inner product
        assert (step >= 0).all() if metric == 0 else (step <= 0).all()
    finally:
        idx.close()


def test_borrowed_device_vectors_and_diag():
    import torch
    data, built, idx = _case(100, 0)
    q = _queries(9, 100, 0)
    want = _search(idx, q, 10, 6, 1, 200, want_diag=True)
    plain = _search(idx, q, 200, 6, 0, 0, want_diag=True)
    assert np.array_equal(want[3], plain[3]) and want[3].any()
    other = rq.IvfRabitqIndex.from_built(built)
    try:
        d_raw = torch.from_numpy(data).to(torch.device("cuda", 0))
        # (a pointer 4 bytes into the allocation: every row of the borrowed array starts off a 16-byte boundary)
        d_off = torch.empty(data.size + 1, dtype=torch.float32, device=d_raw.device)
        d_off[1:] = d_raw.reshape(-1)
        torch.cuda.synchronize()
        for ptr in (d_raw.data_ptr(), d_off.data_ptr() + 4):
            other.set_rerank_vectors(device_ptr=ptr, n=data.shape[0], pool=200)
            ids, sc, cnt, diag = other.batch_search_raw(q, rq.SearchParams(10, 6), want_diag=True)
            _assert_same((ids, sc.view(np.uint32), cnt), want)
            assert np.array_equal(diag, want[3])
    finally:
        other.close()


# ---- every entry ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 5, 300, 1100])
def test_every_entry_agrees(nq):
    """pageable buffers, rbq_host_alloc buffers, two replicas on one device and the device entry on a torch stream return the
    same bits (1100 queries: more than one sub-batch of the host call), and they are the restatement's"""
    import torch
    dim, top_k, nprobe, pool = 20, 10, 6, 64
    data, built, idx = _case(dim, 0)
    q = _queries(nq, dim, 0, seed=2800 + nq)
    want, _ = _restated(idx, data, q, top_k, nprobe, pool, 0)
    base = _search(idx, q, top_k, nprobe, 1, pool)
    _assert_same(base, want, "pageable")
    lib = rq_index.lib()
    idx.set_rerank_pool(pool)
    try:
        nb = [nq * dim * 4, nq * top_k * 8, nq * top_k * 4, nq * 4]
        ptrs = [lib.rbq_host_alloc(b) for b in nb]
        try:
            C.memmove(ptrs[0], q.ctypes.data, nb[0])
            C.memset(ptrs[1], 0xAB, nb[1])
            assert lib.rbq_search_batch(idx._h, ptrs[0], nq, dim, top_k, nprobe, None, 0, ptrs[1], ptrs[2], ptrs[3], None) == 0
            pinned = (np.ctypeslib.as_array(C.cast(ptrs[1], C.POINTER(C.c_uint64)), shape=(nq, top_k)).copy(),
                      np.ctypeslib.as_array(C.cast(ptrs[2], C.POINTER(C.c_uint32)), shape=(nq, top_k)).copy(),
                      np.ctypeslib.as_array(C.cast(ptrs[3], C.POINTER(C.c_uint32)), shape=(nq,)).copy())
        finally:
            for p in ptrs:
                lib.rbq_host_free(p)
        _assert_same(pinned, base, "page-locked")
        dev = torch.device("cuda", 0)
        qd = torch.from_numpy(q).to(dev)
        d_i = torch.zeros(nq, top_k, dtype=torch.int64, device=dev)
        d_s = torch.zeros(nq, top_k, dtype=torch.float32, device=dev)
        d_c = torch.zeros(nq, dtype=torch.int32, device=dev)
        st = torch.cuda.Stream(dev)
        torch.cuda.synchronize(dev)
        idx.search_batch_device(qd.data_ptr(), nq, dim, top_k, nprobe, d_i.data_ptr(), d_s.data_ptr(), d_c.data_ptr(), stream=st.cuda_stream)
        torch.cuda.synchronize(dev)
        idx.release_stream(st.cuda_stream)
        _assert_same((d_i.cpu().numpy().view(np.uint64), d_s.cpu().numpy().view(np.uint32), d_c.cpu().numpy().view(np.uint32)), base, "device entry")
    finally:
        idx.set_rerank_pool(0)
    two = rq.IvfRabitqIndex.from_built(built, devices=[0, 0])
    try:
        assert two.device_count() == 2
        two.set_rerank_vectors(data, pool=pool)
        _assert_same(_search(two, q, top_k, nprobe, 1, pool), base, "two replicas")
    finally:
        two.close()


# ---- off means off ----------------------------------------------------------------------------------------------------
def test_off_means_off():
    data, built, idx = _case(100, 0)
    q = _queries(9, 100, 0)
    for rerank in (0, 1):
        ref = _search(idx, q, 10, 6, rerank, 0)
        for pool in ((5, 10, 64, 4096) if rerank == 0 else (1, 9, 10)):  # rerank off: any pool; rerank on: pool <= top_k
            _assert_same(_search(idx, q, 10, 6, rerank, pool), ref, (rerank, pool))
    for pool in (0, 64, 1025):  # top_k = 1025 with the rerank on stays refused while the pool does not exceed it ...
        with pytest.raises(rq.RabitqError, match="rerank supports top_k <= 1024"):
            _search(idx, q, 1025, 6, 1, pool)
    got = _search(idx, q, 1025, 6, 0, 4096)  # ... and is served as ever with the rerank off
    _assert_same(got, _search(idx, q, 1025, 6, 0, 0))
    with pytest.raises(rq.RabitqError, match="4096"):
        idx.set_rerank_pool(4097)
    assert rq_index.RERANK_POOL_MAX == 4096
    idx.set_rerank_pool(rq_index.RERANK_POOL_MAX)
    for clear in (0, -3, None):  # 0, negative values and None clear it
        idx.set_rerank_pool(64)
        idx.set_rerank_pool(clear)
        idx.set_option("rerank", 1)
        ids, sc, cnt, _ = idx.batch_search_raw(q, rq.SearchParams(10, 6))
        _assert_same((ids, sc.view(np.uint32), cnt), _search(idx, q, 10, 6, 1, 0), clear)
    # the option may be set with no vectors attached, and then has no effect
    bare = rq.IvfRabitqIndex.from_built(built)
    try:
        ref = bare.batch_search_raw(q, rq.SearchParams(10, 6))
        bare.set_rerank_pool(64)
        got = bare.batch_search_raw(q, rq.SearchParams(10, 6))
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)) and np.array_equal(got[2], ref[2])
    finally:
        bare.close()


# ---- recall -----------------------------------------------------------------------------------------------------------
def test_recall_rises_on_a_one_bit_index():
    """1-bit codes, where the estimate is weakest: recall@10 against float64 ground truth with a pool of 200 is no lower than
    without the pool, and strictly higher (fixed seeds; the plain search's recall on them is below 1, checked with the CPU
    oracle: 0.3635 at nprobe 8)."""
    n, dim, nq, top_k, nprobe = 6000, 96, 200, 10, 8
    data, built, idx = _case(dim, 0, n=n, nlist=16, bits=1, seed=2720)
    q = _queries(nq, dim, 0, seed=2830)
    d64 = ((q.astype(np.float64)[:, None, :] - data.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    truth = np.argsort(d64, axis=1, kind="stable")[:, :top_k]

    def recall(ids):
        return sum(len(set(ids[i].tolist()) & set(truth[i].tolist())) for i in range(nq)) / (nq * top_k)

    plain = recall(_search(idx, q, top_k, nprobe, 0, 0)[0])
    unpooled = recall(_search(idx, q, top_k, nprobe, 1, 0)[0])
    pooled = recall(_search(idx, q, top_k, nprobe, 1, 200)[0])
    assert unpooled == plain  # (the unpooled rerank reorders the same ids)
    assert pooled >= plain and pooled > plain, (plain, pooled)
