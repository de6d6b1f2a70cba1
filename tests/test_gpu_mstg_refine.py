"""rbq_mstg_search_refined_batch / _device (include/rbq_mstg.h) on an MI355X.  Every comparison is exact:
the selected lists are select_lists_cpu's, and ids, counts and score bits equal the NumPy restatement over the CPU oracle
(tests/mstg_refine_ref.py; -0.0 and 0.0 are one L2 distance).  Every returned row holds pairwise distinct ids.  Seeded."""
import numpy as np
import pytest
import torch

import mstg_file as mf
import mstg_refine_ref as ref
import oracle
import rabitq_rs_amd as rq
from rabitq_rs_amd import _abi, mstg

pytestmark = pytest.mark.gpu
NONE64 = ref.NONE64


def compare(got, case, q, lists, counts, top_k, refine_pool, cands=None, pair_vec=None):
    """got = (ids, scores, counts[, lists, list_counts]) of the refined call against the restatement"""
    ids, sc, cnt = got[:3]
    if len(got) > 3:
        assert np.array_equal(got[4], counts) and np.array_equal(got[3], lists)
    pv = case.pair_vec if pair_vec is None else pair_vec
    wi, ws, wc, _, ties = ref.refine_ref(case.built, pv, q, lists, counts, case.metric, top_k, refine_pool, cands)
    assert not any(ties)  # (an estimate tie at the pool's cut is decided by the scan's heap: the data must not have one)
    assert np.array_equal(cnt, wc), np.nonzero(cnt != wc)[0][:10]
    bad = np.nonzero((ids != wi).any(axis=1))[0]
    assert bad.size == 0, (bad[:10], ids[bad[0]], wi[bad[0]])
    mask = np.uint32(0x7fffffff if case.metric == 0 else 0xffffffff)
    for i in range(len(q)):
        c = int(cnt[i])
        assert np.array_equal(sc[i, :c].view(np.uint32) & mask, ws[i, :c].view(np.uint32) & mask), i
        assert (ids[i, c:] == NONE64).all() and np.isnan(sc[i, c:]).all(), i
        assert len(set(ids[i, :c].tolist())) == c, i
    return ids, sc, cnt


def run(idx, case, q, top_k, ef, eps, refine_pool, cands=None, **kw):
    lists, counts = rq.select_lists_cpu(q, case.c, ef, eps)
    got = rq.mstg_search(idx, q, top_k, ef, eps, return_lists=True, refine_pool=refine_pool)
    return compare(got, case, q, lists, counts, top_k, refine_pool, cands, **kw)


# ---- the main case ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(b, m) for b in (1, 3, 7) for m in (0, 1)], ids=lambda p: "bits%d_metric%d" % p)
def main(request):
    bits, metric = request.param
    case, q = ref.main_case(bits, metric)
    idx = case.device_index()
    yield case, q, idx
    idx.close()


@pytest.mark.parametrize("eps", [0.6, 1e9])
def test_main_case(main, eps):
    case, q, idx = main
    lists, counts = rq.select_lists_cpu(q, case.c, 6, eps)
    cands = ref.all_candidates(case.built, case.pair_vec, q, lists, counts)
    dup = 0
    for pool in (0, 40, 4096):
        got = rq.mstg_search(idx, q, 10, 6, eps, return_lists=True, refine_pool=pool)
        compare(got, case, q, lists, counts, 10, pool, cands)
        plain = rq.mstg_search(idx, q, max(pool, 10), 6, eps)
        dup += sum(len(set(plain[0][i, :int(plain[2][i])].tolist())) < int(plain[2][i]) for i in range(len(q)))
    assert dup > 0  # the plain call does return ids twice on this data: the refined rows above are unique


def test_counts_and_padding(main):
    case, q, idx = main
    ids, sc, cnt = run(idx, case, q, 400, 1, 0.6, 0)          # one list: fewer distinct ids than top_k
    assert (cnt < 400).all() and (cnt > 0).all()
    run(idx, case, q, 1, 6, 0.6, 40)                          # top_k 1
    if case.metric == 1:  # pool 1 (L2: the queries sit on data points, whose replicas all clamp to 0: a tie at the pool's cut)
        run(idx, case, q, 1, 6, 0.6, 0)
    ids, sc, cnt = run(idx, case, q[:8], 4096, 6, 1e9, 4096)  # top_k = pool = the limit, fewer entries than that
    assert (cnt < 4096).all()
    with pytest.raises(rq.RabitqError) as e:
        rq.mstg_search(idx, q, 10, 6, 0.6, refine_pool=4097)
    assert e.value.code == _abi.RBQ_INVALID_CONFIG and "refine pool too large" in e.value.detail
    z = rq.mstg_search(idx, q, 0, 6, 0.6, return_lists=True, refine_pool=40)
    assert not z[2].any() and not z[4].any()
    z = rq.mstg_search(idx, q, 10, 0, 0.6, return_lists=True, refine_pool=40)
    assert not z[2].any() and (z[0] == NONE64).all() and np.isnan(z[1]).all()


def test_non_finite_queries_select_nothing(main):
    case, q, idx = main
    q = q[:6].copy()
    q[1, 5] = np.nan
    q[4, :] = np.inf
    ids, sc, cnt = run(idx, case, q, 10, 6, 0.6, 40)
    assert cnt[1] == 0 and cnt[4] == 0 and (cnt[[0, 2, 3, 5]] > 0).all()


def test_device_entry_on_a_side_stream_equals_the_host_entry(main):
    case, q, idx = main
    host = rq.mstg_search(idx, q, 10, 6, 0.6, return_lists=True, refine_pool=40)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        tq = torch.from_numpy(q).cuda()
        dev = rq.mstg_search(idx, tq, 10, 6, 0.6, return_lists=True, refine_pool=40)
        short = rq.mstg_search(idx, tq, 10, 6, 0.6, refine_pool=40)
        zero = rq.mstg_search(idx, tq, 10, 0, 0.6, refine_pool=40)
    s.synchronize()
    for a, b in zip(host, dev):
        assert np.array_equal(a.view(np.uint32), b.cpu().numpy().view(np.uint32))
    for a, b in zip(host[:3], short):
        assert np.array_equal(a.view(np.uint32), b.cpu().numpy().view(np.uint32))
    assert not zero[2].cpu().numpy().any() and (zero[0].cpu().numpy() == -1).all()
    idx.release_stream(s.cuda_stream)


def test_result_does_not_depend_on_the_chunk_budget(main):
    case, q, idx = main
    want = rq.mstg_search(idx, q, 10, 6, 0.6, return_lists=True, refine_pool=40)
    tq = torch.from_numpy(q).cuda()
    try:
        for budget in (1, 60_000):
            idx.set_option("mstg_search_budget", budget)
            got = rq.mstg_search(idx, q, 10, 6, 0.6, return_lists=True, refine_pool=40)
            dev = rq.mstg_search(idx, tq, 10, 6, 0.6, return_lists=True, refine_pool=40)
            torch.cuda.synchronize()
            for a, b, d in zip(want, got, dev):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
                assert np.array_equal(a.view(np.uint32), d.cpu().numpy().view(np.uint32))
    finally:
        idx.set_option("mstg_search_budget", 0)


def test_other_handles_return_the_same_rows(main):
    case, q, idx = main
    want = rq.mstg_search(idx, q, 10, 6, 0.6, return_lists=True, refine_pool=40)
    cfg = dict(mf.DEFAULT_CONFIG, rabitq_bits=case.bits, faster_config=True, metric=case.metric, closure_epsilon=2.0)
    loaded, _ = mstg.load_mstg(mstg.save_mstg_bytes(idx, cfg))
    from_built = rq.IvfRabitqIndex.from_built(case.built_with_real_ids())
    for h in (loaded, from_built):
        got = rq.mstg_search(h, q, 10, 6, 0.6, return_lists=True, refine_pool=40)
        for a, b in zip(want, got):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        h.close()


# ---- shapes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [7, 3])
@pytest.mark.parametrize("dim", [16, 48, 960, 2048])
def test_dimensions(dim, bits):
    import closure_cases as cc
    x, c = cc.clustered(300, dim, 8, 500 + dim)
    case = ref.Case(x, c, bits, 0, 2.0, 8)
    rng = np.random.default_rng(dim)
    q = (x[rng.integers(0, 300, 12)] + 0.01 * rng.standard_normal((12, dim))).astype(np.float32)
    idx = case.device_index()
    lists, counts = rq.select_lists_cpu(q, case.c, 4, 0.6)
    cands = ref.all_candidates(case.built, case.pair_vec, q, lists, counts)
    for pool in (40, 4096):
        got = rq.mstg_search(idx, q, 10, 4, 0.6, return_lists=True, refine_pool=pool)
        compare(got, case, q, lists, counts, 10, pool, cands)
    idx.close()


@pytest.mark.parametrize("bits,metric", [(7, 0), (3, 1), (1, 0)])
def test_list_lengths_0_1_32_33(bits, metric):
    case, q = ref.list_length_case(bits, metric)
    idx = rq.IvfRabitqIndex.from_built(case.built_with_real_ids())
    for pool in (0, 4096):
        ids, sc, cnt = run(idx, case, q, 10, 4, 1e9, pool)
    assert (cnt == 10).all()
    ids, sc, cnt = run(idx, case, q, 100, 4, 1e9, 0)
    assert (cnt == 66).all()  # every vector of the index, once
    idx.close()


@pytest.mark.parametrize("bits,metric", [(7, 0), (3, 1), (1, 0)])
def test_exact_ties_are_ordered_by_rank(bits, metric):
    case, q = ref.exact_tie_case(bits, metric)
    idx = rq.IvfRabitqIndex.from_built(case.built_with_real_ids())
    ids, sc, cnt = run(idx, case, q, 120, 4, 1e9, 4096)  # pool > candidates: every entry is refined
    assert (cnt == 120).all()
    # the twins that share a list come back next to each other with equal distances, the earlier vector first
    m, pairs = 60, 0
    for i in range(len(q)):
        pos = {int(v): p for p, v in enumerate(ids[i])}
        for v in range(0, m, 2):
            a, b = pos[v], pos[v + m]
            assert sc[i, a] == sc[i, b] and a < b
            pairs += 1
    assert pairs
    run(idx, case, q, 10, 4, 1e9, 4096)
    idx.close()


def test_numeric_variant_native_avx2():
    """the handle's variant reaches the ex-code dot of the refinement: against the oracle in the same variant"""
    case, q = ref.main_case(7, 0)
    idx = case.device_index()
    idx.set_numeric_variant("native_avx2")
    base = rq.mstg_search(idx, q, 10, 6, 0.6, refine_pool=40)
    with oracle.variant("ex_avx2"):
        ids, sc, cnt = run(idx, case, q, 10, 6, 0.6, 40)
    idx.set_numeric_variant("native_avx512")
    dflt = rq.mstg_search(idx, q, 10, 6, 0.6, refine_pool=40)
    print("queries whose score bits differ between the variants:", int((dflt[1].view(np.uint32) != sc.view(np.uint32)).any(axis=1).sum()), "of", len(q))
    assert np.array_equal(base[1].view(np.uint32), sc.view(np.uint32))
    idx.close()


# ---- the binding ----------------------------------------------------------------------------------------------------------------
def test_binding():
    import closure_cases as cc
    x, _ = cc.clustered(600, 32, 8, 900)
    m = mstg.MstgIndex(32, "euclidean", max_posting_size=40, branching_factor=4, closure_epsilon=2.0, rabitq_bits=7, default_ef_search=6)
    m.fit(x)
    assert m.refine_pool is None
    q = x[:20] + np.float32(0.01)
    plain = m.batch_query(q, 10)
    ids, dist, cnt = rq.mstg_search(m.handle, q, 10, 6, 0.6)  # refine_pool=None: the existing call, bit for bit
    i2, d2, c2 = rq.mstg_search(m.handle, q, 10, 6, 0.6, refine_pool=None)
    assert np.array_equal(ids, i2) and np.array_equal(dist.view(np.uint32), d2.view(np.uint32)) and np.array_equal(cnt, c2)
    for i, row in enumerate(plain):
        assert np.array_equal(row[:, 1].view(np.uint32), dist[i, :cnt[i]].view(np.uint32))
        assert np.array_equal(row[:, 0], ids[i, :cnt[i]].astype(np.float32))
    assert any(len(set(r[:, 0].tolist())) < len(r) for r in plain)  # (this data does return ids twice)
    m.set_query_arguments(refine_pool=40)
    assert m.refine_pool == 40 and m.default_ef_search == 6
    refined = m.batch_query(q, 10)
    ri, rd, rc = rq.mstg_search(m.handle, q, 10, 6, 0.6, refine_pool=40)
    for i, row in enumerate(refined):
        assert len(set(row[:, 0].tolist())) == len(row) == rc[i]
        assert np.array_equal(row[:, 1].view(np.uint32), rd[i, :rc[i]].view(np.uint32))
    one = m.query(q[0], 10)
    assert np.array_equal(one, refined[0])
    m.set_query_arguments(ef_search=5)
    assert m.refine_pool == 40
    m.set_query_arguments(refine_pool=None)
    assert m.refine_pool is None
    again = m.batch_query(q, 10)
    m.set_query_arguments(ef_search=6)
    again = m.batch_query(q, 10)
    assert all(np.array_equal(a, b) for a, b in zip(plain, again))


# ---- recall, for the record -------------------------------------------------------------------------------------------------------
def test_recall_refined_is_not_below_plain():
    """7 bits, L2, pool 100: recall@10 against exact float distances, counting distinct ids (figures: DESIGN.md section 19)"""
    case, q = ref.recall_case()
    idx = case.device_index()
    d2 = ((q[:, None, :].astype(np.float64) - case.x[None, :, :].astype(np.float64)) ** 2).sum(-1)
    truth = np.argsort(d2, axis=1, kind="stable")[:, :10].astype(np.uint64)
    pi, _, pc = rq.mstg_search(idx, q, 10, 16, 0.6)
    ids, sc, cnt = run(idx, case, q, 10, 16, 0.6, 100)
    plain, refined = ref.recall_at(pi, pc, truth), ref.recall_at(ids, cnt, truth)
    print(f"recall@10: plain {plain:.4f} refined (pool 100) {refined:.4f}")
    assert refined >= plain
    idx.close()
