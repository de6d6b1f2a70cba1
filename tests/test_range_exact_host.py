"""tests/range_exact_ref.py (the exact range search restated) without a GPU: the restatement against a
direct pass over the probed vectors, and that the cases tests/test_gpu_range_exact.py runs are worth running — the exact test
rejects candidates, a narrower candidate radius loses matches, some query has none.  The case is test_gpu_range's: n 3000, 12
lists, nprobe 6, 7 generator queries and the far one, dim 64."""
import functools

import numpy as np
import pytest

import range_exact_ref as xref
import range_ref
from rerank_pool_ref import exact_scores
from test_gpu_range import _case

F32 = np.float32
NPROBE = 6


def _subsequence(a, b):
    """a is b with entries left out, in b's order"""
    it = iter(b.tolist())
    return all(any(x == y for y in it) for x in a.tolist())


@functools.lru_cache(maxsize=None)
def _results(metric, bits):
    data, built, q = _case(metric, bits, 64)
    x = xref.kth_exact_score(built, q[0], data, 21, NPROBE)
    radii = [range_ref.kth_distance_radius(built, q[0], 21, NPROBE), range_ref.kth_distance_radius(built, q[0], 50, NPROBE),
             xref.unbounded_radius(metric)]
    cands = [range_ref.range_batch(built, q, r, NPROBE) for r in radii]
    exact = [[xref.from_candidates(c, qq, data, x, metric) for c, qq in zip(cand, q)] for cand in cands]
    return data, built, q, x, radii, cands, exact


@pytest.mark.parametrize("bits", [1, 3, 7])
@pytest.mark.parametrize("metric", [0, 1], ids=["L2", "IP"])
def test_the_cases_exercise_the_exact_step(metric, bits):
    data, built, q, x, radii, cands, exact = _results(metric, bits)
    n_cand = [[len(c[0]) for c in cand] for cand in cands]
    n_match = [[len(e[0]) for e in ex] for ex in exact]
    print("candidates", n_cand, "matches", n_match)
    assert min(n_match[2]) == 0, "no query without a match"
    assert sum(n_cand[0]) > sum(n_match[0]), "the exact test rejects nothing at the estimate's 21st distance"
    assert n_match[2][0] == 20, "query 0 at the unbounded candidate radius: the 20 vectors nearer than its 21st"
    # the batch's totals at the estimate's 50th distance against its 21st: more candidates in every case; matches never fewer (the
    # narrower result is a subsequence), and strictly more at 1 bit, where the estimate is off by tens of per cent — at 7 bits it is
    # off by a few per mille, and the L2 case loses no match at the narrower radius (65 and 65)
    assert sum(n_cand[1]) > sum(n_cand[0]), "the wider candidate radius admits no more"
    assert sum(n_match[1]) >= sum(n_match[0])
    if bits == 1:
        assert sum(n_match[1]) > sum(n_match[0]), "the wider candidate radius finds no more"
    # the estimate's matches are only candidates: the restatement's result is what rule 3 leaves of them, with the candidate scan's counters
    for cand, ex in zip(cands, exact):
        for c, e in zip(cand, ex):
            assert e[2] == c[2] and _subsequence(e[0], c[0])
            assert xref.passes(e[1], x, metric).all()


@pytest.mark.parametrize("bits", [1, 3, 7])
@pytest.mark.parametrize("metric", [0, 1], ids=["L2", "IP"])
def test_narrower_candidates_give_a_subsequence(metric, bits):
    data, built, q, x, radii, cands, exact = _results(metric, bits)
    for narrow, wide in ((0, 1), (1, 2), (0, 2)):
        for a, b in zip(exact[narrow], exact[wide]):
            assert _subsequence(a[0], b[0])
            score_of = dict(zip(b[0].tolist(), b[1].view(np.uint32).tolist()))
            assert [score_of[i] for i in a[0].tolist()] == a[1].view(np.uint32).tolist()


@pytest.mark.parametrize("bits", [1, 3, 7])
@pytest.mark.parametrize("metric", [0, 1], ids=["L2", "IP"])
def test_unbounded_candidates_are_a_direct_pass(metric, bits):
    """r = +inf (L2) / -inf (inner product): every probed vector the loop evaluates to a finite distance is a candidate, so the
    result is rule 3 over the probed vectors, list by list"""
    data, built, q, x, radii, cands, exact = _results(metric, bits)
    for qq, got in zip(q, exact[2]):
        ids, sc = [], []
        for pid, _, d in range_ref.probed_vectors(built, qq, NPROBE):
            pid = pid[np.isfinite(d)]
            ex = exact_scores(qq, data, pid, metric)
            keep = ex < x if metric == 0 else ex > x
            ids.append(pid[keep])
            sc.append(ex[keep])
        assert np.array_equal(np.concatenate(ids), got[0])
        assert np.array_equal(np.concatenate(sc).view(np.uint32), got[1].view(np.uint32))


def test_batch_entry_widening_and_rows():
    """range_exact_batch is range_query + exact_scores + rule 3; 16-bit rows enter widened; rows() pads and counts past the capacity"""
    import rerank_f16_ref
    data, built, q, x, radii, cands, exact = _results(0, 3)
    got = xref.range_exact_batch(built, q, data, x, radii[1], NPROBE)
    for a, b in zip(got, exact[1]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and a[2] == b[2]
    h = rerank_f16_ref.round_to(data, "f16")
    w = xref.widened(h, "f16")
    assert w.dtype == F32 and np.array_equal(w, h.view(np.float16).astype(F32)) and not np.array_equal(w, data)
    assert np.array_equal(xref.widened(rerank_f16_ref.round_to(data, "bf16"), "bf16").view(np.uint32) & 0xFFFF, np.zeros(data.shape, np.uint32))
    half = xref.range_exact_batch(built, q, data[:1500], x, radii[2], NPROBE)  # ids without a raw row score NaN: never a match
    for a, b in zip(half, exact[2]):
        assert (a[0] < 1500).all() and np.array_equal(a[0], b[0][b[0] < 1500])
    tot = [len(e[0]) for e in exact[2]]
    cap = max(tot) - 1
    ids, bits, totals = xref.rows(exact[2], cap)
    assert totals.tolist() == tot and (ids[0, tot[0]:] == range_ref.PAD_ID).all() and (bits[0, tot[0]:] == range_ref.PAD_SCORE_BITS).all()
    assert np.array_equal(ids[int(np.argmax(tot))], exact[2][int(np.argmax(tot))][0][:cap])
