"""The exact brute-force top-k with the pool chosen by rank (rbq_bf_search_exact_ranked_batch: k_bf_dist -> k_bf_pool_hist x 4 ->
k_bf_pool_count -> k_bf_pool_place -> k_bf_rerank_score -> k_bf_rerank_order) against its restatement
(tests/bf_pool_rank_ref.py), every comparison exact: ids, score bits, counts and the unused slots of every row.  Seeded."""
import functools

import numpy as np
import pytest

import rabitq_rs_amd as rq
from rabitq_rs_amd import _abi, bruteforce as bfm
import bf_pool_rank_ref as ref
import bf_range_exact_ref as xref
import bf_ref

pytestmark = pytest.mark.gpu
POOLS = (None, 100, 129, 2048, 4096)  # top_k itself; below a span; past the score kernel's slice; a span; the largest (two carried blocks)
# (n, dim, bits, metric, raw, rows scaled by 2^-10 .. 2^10): 1100 is one partial span, 4500 three spans with the last partial.  The
# scaled rows spread the estimates over twenty exponents, the inner product over both signs: pool boundaries fall where keys differ
# in the sign bit, the exponent bytes and the low bytes, so every radix pass decides something.
KEYS = [(1100, 20, 7, 0, "f32", False), (1100, 33, 1, 1, "f16", False), (4500, 33, 1, 0, "f16", False), (4500, 20, 7, 1, "f32", False),
        (1100, 33, 7, 1, "f16", True), (4500, 20, 7, 0, "f32", True), (4500, 33, 1, 1, "f32", True)]
KEY = KEYS[0]
DUPS = (5, 2050, 2051, 4100, 4499)  # copies of one row in all three spans of 4500 vectors, on both sides of vectors 2048 and 2049
NEARER = 3000


@functools.lru_cache(maxsize=None)
def case(n, dim, bits, metric, scaled=False, nq=5, ties=None):
    """(index, prep, queries near data rows, data, the builder's result: prep rotates queries with its header, so it stays alive).
    ties "dups": rows DUPS are one row and every query is that row plus noise; "nearer": row NEARER is nearer to query 0 still."""
    rng = np.random.default_rng(1000 * bits + 10 * metric + dim + n)
    data = (rng.standard_normal((n, dim)) + 1.0).astype(np.float32)
    if scaled:
        data *= np.exp2(rng.integers(-10, 11, n)).astype(np.float32)[:, None]
    noise = rng.standard_normal((nq, dim)).astype(np.float32)
    if ties:
        data[list(DUPS)] = data[DUPS[0]]
        q = data[DUPS[0]] + np.float32(0.3) * noise
        if ties == "nearer":
            data[NEARER] = data[DUPS[0]] + np.float32(0.27) * noise[0]
    else:
        q = data[rng.integers(0, n, nq)] * (1.0 + 0.3 * noise)
    built = rq.builder.train_bruteforce(data, bits, metric, 1, 7, True)
    return rq.BruteForceRabitqIndex.from_built(built), bf_ref.Prepared(built.hdr_ptr, built.arrays()), q.astype(np.float32), data, built


def attached(key, **kw):
    """(the case's index with its data attached in key's element type, prep, queries, the rows the scorer sees)"""
    idx, prep, q, data = case(*key[:4], *key[5:], **kw)[:4]
    stored, dtype, wide = xref.stored_rows(data, key[4])
    idx.set_rerank_vectors(stored, dtype=dtype)
    return idx, prep, q, wide


def run(idx, q, k, pool, chunk=0, words=None, nbits=0, rule="rank"):
    """(ids, score bits, counts) with at most `chunk` vectors per chunk (0: no limit); the call launches no k_bf_select under "rank\""""
    L = bfm.lib()
    assert L.rbq_bf_debug_set_chunk_vectors(chunk) == 0
    try:
        l0 = L.rbq_bf_debug_select_launches()
        ids, sc, cnt = idx.batch_search_exact_raw(q, rq.BruteForceSearchParams(k), pool, words, nbits, pool_rule=rule)
        assert rule == "heap" or L.rbq_bf_debug_select_launches() == l0
        return ids, sc.view(np.uint32), cnt
    finally:
        L.rbq_bf_debug_set_chunk_vectors(0)


def same(got, want):
    return all(a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want))


@pytest.mark.parametrize("key", KEYS, ids=str)
def test_parity(key):
    idx, prep, q, wide = attached(key)
    for pool in POOLS:
        want, pcount = ref.rows(prep, q, wide, 10, pool)
        assert (pcount == min(key[0], pool or 10)).all()  # (pool 4096 of 1100 vectors: every candidate comes back)
        assert same(run(idx, q, 10, pool), want), pool


@pytest.mark.parametrize("ties,k", [(t, k) for t in ("dups", "nearer") for k in (1, 3, 4)])
def test_ties_at_the_pool_boundary_go_to_the_smallest_ids(ties, k):
    """top_k = pool = k cuts the group of equal estimates: the output is the whole pool"""
    key = (4500, 20, 7, 0, "f32", False)
    idx, prep, q, wide = attached(key, ties=ties)
    d0 = bf_ref.distances(prep, q[0])
    assert len(set(d0[list(DUPS)].view(np.uint32))) == 1 and (np.delete(d0, DUPS + (NEARER,)) > d0[DUPS[0]]).all()
    lead = ((NEARER,) if ties == "nearer" and d0[NEARER] < d0[DUPS[0]] else ()) + DUPS
    assert ties == "dups" or lead[0] == NEARER
    want = ref.rows(prep, q, wide, k, k)[0]
    assert sorted(want[0][0].tolist()) == sorted(lead[:k])
    assert same(run(idx, q, k, k), want)


@pytest.mark.parametrize("left", [6, 0])
def test_filter_leaves_fewer_than_top_k(left):
    idx, prep, q, wide = attached(KEY)
    allowed = np.zeros(KEY[0], bool)
    allowed[np.random.default_rng(5).choice(900, left, replace=False)] = True
    words, nbits = bfm._filter_words(np.nonzero(allowed)[0])
    want = ref.rows(prep, q, wide, 10, 100, allowed)[0]
    assert (want[2] == left).all() and (want[0][:, left:] == ref.U64MAX).all() and (want[1][:, left:] == ref.NAN_BITS).all()
    assert same(run(idx, q, 10, 100, 0, words, nbits), want)


def test_a_query_with_a_non_finite_component_has_no_candidate():
    idx, prep, q, wide = attached(KEY)
    q = q.copy()
    q[1, 3] = np.inf
    want = ref.rows(prep, q, wide, 10, 100)[0]
    assert want[2][1] == 0 and want[2][0] == 10
    assert same(run(idx, q, 10, 100), want)


@pytest.mark.parametrize("chunk", [512, 2048, 2049])
def test_chunks_of_vectors_do_not_change_the_bytes(chunk):
    idx, prep, q, wide = attached((4500, 20, 7, 0, "f32", False), ties="dups")
    for k, pool in ((3, 3), (4, 4), (10, 100), (10, 4096)):
        whole = run(idx, q, k, pool)
        assert same(whole, ref.rows(prep, q, wide, k, pool)[0]) and same(run(idx, q, k, pool, chunk), whole), (k, pool)


def test_a_second_sub_batch():
    idx, prep, q, wide = attached((300, 7, 7, 0, "bf16", False, 1030))  # 1030 queries: the plan's sub-batch is 1024
    assert same(run(idx, q, 10, 20), ref.rows(prep, q, wide, 10, 20)[0])


def test_other_calls_untouched_the_same_bytes_twice_and_the_python_layer():
    idx, prep, q, wide = attached(KEY)
    p = rq.BruteForceSearchParams(10)
    before, heap_before, stats = idx.batch_search_raw(q, p), run(idx, q, 10, 129, rule="heap"), idx.heap_stats()
    got = run(idx, q, 10, 129)
    assert idx.heap_stats() == stats
    assert same(got, ref.rows(prep, q, wide, 10, 129)[0]) and same(run(idx, q, 10, 129), got)
    assert same(got, heap_before)  # (no equal estimates in this data: both rules form one pool)
    assert same(idx.batch_search_raw(q, p), before) and same(run(idx, q, 10, 129, rule="heap"), heap_before)
    res = idx.batch_search_exact(q, p, pool=129, pool_rule="rank")
    assert [[r.id for r in row] for row in res] == got[0].tolist() and res[0] == idx.search_exact(q[0], p, pool=129, pool_rule="rank")
    assert sorted(r.id for r in idx.search_exact(q[0], p, 129, allowed_ids=[5, 3], pool_rule="rank")) == [3, 5]
    with pytest.raises(ValueError, match="pool_rule"):
        idx.batch_search_exact_raw(q, p, pool_rule="radix")


def test_without_raw_vectors_the_call_is_refused():
    q, data = case(*KEY[:4])[2:4]
    idx = rq.BruteForceRabitqIndex.train(data, KEY[2], KEY[3], 1, 7, True)
    with pytest.raises(rq.RabitqError, match=r"exact search needs raw vectors attached \(rbq_bf_set_rerank_vectors\)") as e:
        idx.batch_search_exact_raw(q, rq.BruteForceSearchParams(10), pool=100, pool_rule="rank")
    assert e.value.code == _abi.RBQ_INVALID_CONFIG
    idx.close()
