"""rbq_mstg_search_batch / rbq_mstg_search_batch_device (include/rbq_mstg.h) on an MI355X.  Two assertions hold for every case
(tests/mstg_search_cases.py): the selected lists equal select_lists_cpu, and ids, counts and score bits equal both the oracle's
posting-list scan and rbq_posting_scan_batch fed those lists.  Deterministic and seeded."""
import numpy as np
import pytest
import torch

import mstg_search_cases as mc
import rabitq_rs_amd as rq
from rabitq_rs_amd import _abi, mstg

pytestmark = pytest.mark.gpu


def _run(built, cent, q, metric, top_ks=(10, 100), efs=(150,), epss=(0.6,)):
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        for top_k in top_ks:
            for ef in efs:
                for eps in epss:
                    mc.check(idx, built, cent, q, top_k, ef, eps, metric)
    finally:
        idx.close()


@pytest.mark.parametrize("bits", [1, 3, 7])
@pytest.mark.parametrize("metric", [0, 1])
def test_metrics_and_bits(metric, bits):
    built, cent, q = mc.kmeans_case(metric, bits, 128, 6000, 48, 40, 31 + bits)
    # 7000 is above the candidate count of any query
    _run(built, cent, q, metric, top_ks=(10, 100, 7000), efs=(150, 5), epss=(0.6, 0.05))


@pytest.mark.parametrize("dim", [16, 960, 2048])
def test_dimensions(dim):
    built, cent, q = mc.kmeans_case(0, 7, dim, 3000, 48, 24, 40 + dim)
    _run(built, cent, q, 0, efs=(150, 7), epss=(0.6, 0.1))


@pytest.mark.parametrize("nlist", [1, 2, 256, 257, 1024])
def test_list_counts(nlist):
    built, cent, q = mc.kmeans_case(0, 3, 64, 5000, nlist, 40, 50 + nlist)
    _run(built, cent, q, 0, efs=(0, 1, 150, nlist, nlist + 7), epss=(0.6, 1e9, -0.5, float("nan"), 0.0))


def test_1024_lists_960_dims_takes_the_shortlist():
    nq = 64
    built, cent, q = mc.kmeans_case(0, 7, 960, 8000, 1024, nq, 77)
    before = mstg.search_fallbacks()
    _run(built, cent, q, 0, top_ks=(10,), efs=(150,), epss=(0.6,))
    fb = mstg.search_fallbacks() - before
    print("fallback queries:", fb, "of", nq)
    assert fb < nq  # the shortlist path is really exercised
    _run(built, cent, q, 0, top_ks=(100,), efs=(300, 50), epss=(0.8, 0.4))
    built, cent, q = mc.kmeans_case(1, 7, 960, 8000, 1024, 32, 78)
    _run(built, cent, q, 1, top_ks=(10,), efs=(150,), epss=(0.6,))


def test_twenty_thousand_short_lists():
    built, cent, q = mc.pair_case(0, 1, 32, 20000, 48, 91)
    before = mstg.search_fallbacks()
    _run(built, cent, q, 0, efs=(150, 300), epss=(0.6, 1e9))
    print("fallback queries:", mstg.search_fallbacks() - before)


def test_duplicated_centroids():
    """every centroid twice: ties at every rank, the cut at ef included"""
    rng = np.random.default_rng(3)
    base = rng.standard_normal((300, 64)).astype(np.float32) * 2
    cent = np.concatenate([base, base])
    data = (base[rng.integers(0, 300, 3000)] + 0.2 * rng.standard_normal((3000, 64))).astype(np.float32)
    built = mc.given_centroids_case(3, data, cent, 4)
    q = data[:32] + np.float32(0.01)
    _run(built, cent, q, 0, top_ks=(10,), efs=(1, 2, 7, 150, 301), epss=(0.6, 1e9))


def test_permuted_centroids():
    """centroids that are coordinate permutations of query + offset: every S is equal up to the order of summation"""
    rng = np.random.default_rng(9)
    dim, k = 64, 400
    q0 = rng.standard_normal(dim).astype(np.float32)
    v = q0 + rng.standard_normal(dim).astype(np.float32)
    delta = v - q0
    cent = np.stack([q0 + delta[rng.permutation(dim)] for _ in range(k)]).astype(np.float32)
    data = (cent[rng.integers(0, k, 2000)] + 0.1 * rng.standard_normal((2000, dim))).astype(np.float32)
    built = mc.given_centroids_case(7, data, cent, 10)
    q = np.stack([q0] * 4 + [q0 + np.float32(1e-3) * rng.standard_normal(dim).astype(np.float32) for _ in range(12)]).astype(np.float32)
    _run(built, cent, q, 0, top_ks=(10,), efs=(1, 50, 150), epss=(0.6, 0.0, 1e-6))


def test_a_common_offset_falls_back_and_still_matches():
    """data + 300: eps is larger than the spread of the distances, the shortlist of 2500 centroids overflows, queries fall back"""
    built, cent, q = mc.pair_case(0, 3, 48, 2500, 32, 17, offset=300.0)
    before = mstg.search_fallbacks()
    _run(built, cent, q, 0, top_ks=(10,), efs=(150, 2500), epss=(0.6,))
    fb = mstg.search_fallbacks() - before
    print("fallback queries:", fb)
    assert fb > 0


def test_non_finite_queries_select_nothing():
    built, cent, q = mc.kmeans_case(0, 3, 64, 4000, 300, 16, 23)
    q[3, 5] = np.nan
    q[7, 0] = np.inf
    idx = rq.IvfRabitqIndex.from_built(built)
    ids, sc, cnt, li, lc = rq.mstg_search(idx, q, 10, 150, 0.6, return_lists=True)
    rl, rc = rq.select_lists_cpu(q, cent, 150, 0.6)
    assert np.array_equal(lc, rc) and np.array_equal(li, rl) and lc[3] == 0 and lc[7] == 0 and cnt[3] == 0 and cnt[7] == 0
    pids, psc, pcnt = idx.posting_scan(q, 10, rl, rc)
    assert np.array_equal(cnt, pcnt) and np.array_equal(ids, pids) and np.array_equal(sc.view(np.uint32), psc.view(np.uint32))
    idx.close()


def test_device_entry_on_a_side_stream_equals_the_host_entry():
    built, cent, q = mc.kmeans_case(0, 7, 128, 6000, 400, 200, 61)
    idx = rq.IvfRabitqIndex.from_built(built)
    host = rq.mstg_search(idx, q, 10, 150, 0.6, return_lists=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        tq = torch.from_numpy(q).cuda()
        dev = rq.mstg_search(idx, tq, 10, 150, 0.6, return_lists=True)
        short = rq.mstg_search(idx, tq, 10, 150, 0.6)
    s.synchronize()
    assert np.array_equal(dev[0].cpu().numpy().view(np.uint64), host[0])
    assert np.array_equal(dev[1].cpu().numpy().view(np.uint32), host[1].view(np.uint32))
    assert np.array_equal(dev[2].cpu().numpy().view(np.uint32), host[2])
    assert np.array_equal(dev[3].cpu().numpy().view(np.uint32), host[3])
    assert np.array_equal(dev[4].cpu().numpy().view(np.uint32), host[4])
    assert np.array_equal(short[0].cpu().numpy().view(np.uint64), host[0]) and np.array_equal(short[2].cpu().numpy().view(np.uint32), host[2])
    # ef_search = 0 and top_k = 0 on the device entry
    with torch.cuda.stream(s):
        z = rq.mstg_search(idx, tq, 10, 0, 0.6, return_lists=True)
        t0 = rq.mstg_search(idx, tq, 0, 150, 0.6, return_lists=True)
    s.synchronize()
    assert not z[2].cpu().numpy().any() and (z[0].cpu().numpy() == -1).all() and np.isnan(z[1].cpu().numpy()).all() and not z[4].cpu().numpy().any()
    assert not t0[2].cpu().numpy().any() and not t0[4].cpu().numpy().any()
    idx.close()


def test_result_does_not_depend_on_the_chunk_budget():
    built, cent, q = mc.kmeans_case(0, 3, 64, 5000, 300, 150, 71)
    idx = rq.IvfRabitqIndex.from_built(built)
    want = rq.mstg_search(idx, q, 10, 150, 0.6, return_lists=True)
    tq = torch.from_numpy(q).cuda()
    for budget in (1, 200_000, 3_000_000):
        idx.set_option("mstg_search_budget", budget)
        got = rq.mstg_search(idx, q, 10, 150, 0.6, return_lists=True)
        for a, b in zip(want, got):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        dev = rq.mstg_search(idx, tq, 10, 150, 0.6, return_lists=True)
        torch.cuda.synchronize()
        for a, b in zip(want, dev):
            assert np.array_equal(a.view(np.uint32), b.cpu().numpy().view(np.uint32))
    idx.close()


def test_posting_scan_does_not_depend_on_its_own_chunks():
    """rbq_posting_scan_batch cuts a call into chunks of 16384 queries: one call over 16384 + 5 queries (two chunks) equals two
    calls over the rows of each chunk.  Lists of 0, 1, 32 and 33 vectors; the queries of the second chunk name the longest twice."""
    rng = np.random.default_rng(101)
    lens, dim, cut = (0, 1, 32, 33), 16, 16384
    nq = cut + 5
    assign = np.repeat(np.arange(4), lens).astype(np.uint32)
    cent = (rng.standard_normal((4, dim)) * 3).astype(np.float32)
    data = (cent[assign] + 0.3 * rng.standard_normal((len(assign), dim))).astype(np.float32)
    built = rq.builder.train_with_clusters(data, cent, assign, 3, 0, rq.RotatorType.NoRotation, 101, True)
    q = (data[rng.integers(0, len(data), nq)] + 0.2 * rng.standard_normal((nq, dim))).astype(np.float32)
    lists = np.tile(np.arange(4, dtype=np.uint32), (nq, 1))
    lists[cut:, 0] = 3
    counts = np.full(nq, 4, np.uint32)
    idx = rq.IvfRabitqIndex.from_built(built)
    ids, sc, cnt = idx.posting_scan(q, 3, lists, counts)
    assert (cnt == 3).all()  # (every query scans at least the 32 + 33 vectors of lists 2 and 3)
    for rows in (slice(0, cut), slice(cut, nq)):
        pids, psc, pcnt = idx.posting_scan(q[rows], 3, lists[rows], counts[rows])
        assert np.array_equal(cnt[rows], pcnt) and np.array_equal(ids[rows], pids)
        assert np.array_equal(sc[rows].view(np.uint32), psc.view(np.uint32))
    idx.close()


def test_handle_built_on_the_device_is_searched_end_to_end():
    rng = np.random.default_rng(12)
    cent = (rng.standard_normal((300, 64)) * 3).astype(np.float32)
    data = (cent[rng.integers(0, 300, 6000)] + rng.standard_normal((6000, 64))).astype(np.float32)
    idx = rq.build_postings_on_device(data, cent, 7, 0, closure_epsilon=0.15, max_replicas=8, faster_config=True)
    q = (data[:64] + 0.05 * rng.standard_normal((64, 64))).astype(np.float32)
    for p in (rq.MstgSearchParams.balanced(), rq.MstgSearchParams.high_recall(), rq.MstgSearchParams.low_latency()):
        ids, sc, cnt, li, lc = mc.check(idx, None, cent, q, 10, p.ef_search, p.pruning_epsilon, 0)
        assert (cnt > 0).all()
    # the query's own vector is in the lists searched
    assert np.mean([i in ids[i, :int(cnt[i])] for i in range(64)]) > 0.9
    idx.close()


def test_errors():
    from conftest import build_index
    data, built = build_index(n=500, dim=64, nlist=4, total_bits=7)
    rot = rq.IvfRabitqIndex.from_built(built)
    with pytest.raises(rq.RabitqError) as e:
        rq.mstg_search(rot, data[:2], 5)
    assert e.value.code == _abi.RBQ_INVALID_CONFIG
    rot.close()
    built, cent, q = mc.kmeans_case(0, 3, 64, 2000, 20, 8, 5)
    idx = rq.IvfRabitqIndex.from_built(built)
    with pytest.raises(rq.RabitqError) as e:
        rq.mstg_search(idx, q[:, :48], 5)
    assert e.value.code == _abi.RBQ_DIMENSION_MISMATCH
    ids, sc, cnt, li, lc = rq.mstg_search(idx, q, 0, 150, 0.6, return_lists=True)
    assert not cnt.any() and not lc.any()
    ids, sc, cnt, li, lc = rq.mstg_search(idx, q, 5, 0, 0.6, return_lists=True)
    assert not cnt.any() and not lc.any() and li.shape == (8, 0) and (ids == mc.NONE64).all() and np.isnan(sc).all()
    idx.close()
