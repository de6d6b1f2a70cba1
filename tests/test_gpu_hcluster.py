"""MSTG hierarchical balanced clustering on the GPU (rbq_mstg_cluster_device): every array equals the CPU restatement
(rbq_build_hcluster) bit for bit on the smallest shapes that reach each path (tests/hcluster_cases.py), wherever a split runs
(`host_below`) and wherever the data lives; and `MstgIndex.fit` strings clustering, closure assignment and encoding together."""
import numpy as np
import pytest
import torch

import hcluster_cases as hc
import rabitq_rs_amd as rq
from rabitq_rs_amd import _abi

pytestmark = pytest.mark.gpu


def _gpu(name, **kw):
    x, mps, k, w, it = hc.cases()[name]
    return rq.hierarchical_cluster(x, mps, k, w, it, **kw)


@pytest.mark.parametrize("name", sorted(hc.cases()))
def test_device_equals_cpu_restatement(name):
    want = hc.cpu(name)
    if name == hc.BALANCING:
        assert want[3]["balance_moves"] > 0
    if name in hc.IDENTICAL:
        assert want[3]["empty_reseeded"] > 0 and want[3]["balance_moves"] > 0
    if name == "identical_60_k12":
        assert want[3]["rng_draws"] > 0
    got = _gpu(name, host_below=0)
    hc.same(got, want)
    for s in ("splits", "balance_moves", "empty_reseeded", "rng_draws"):
        assert got[3][s] == want[3][s], (s, got[3], want[3])
    assert got[3]["host_splits"] == 0 and got[3]["arena_bytes"] > 0


@pytest.mark.parametrize("name", [hc.SAMPLED, hc.BALANCING, "identical_60_k12", "odd_dim_13"])
def test_result_does_not_depend_on_host_below(name):
    want = hc.cpu(name)
    res = {hb: _gpu(name, host_below=hb) for hb in (0, 64, 400, 10 ** 9)}
    for hb, got in res.items():
        hc.same(got, want)
        for s in ("splits", "balance_moves", "empty_reseeded", "rng_draws"):
            assert got[3][s] == want[3][s], (hb, s, got[3], want[3])
    splits = want[3]["splits"]
    assert res[0][3]["host_splits"] == 0
    assert res[10 ** 9][3]["host_splits"] == splits
    assert 0 <= res[64][3]["host_splits"] <= res[400][3]["host_splits"] <= splits
    if name == hc.SAMPLED:
        # 64 is below this case's max_posting_size (100): such clusters are final, so nothing is handed over; at 400 the root
        # (1500 rows) splits on the device and subtrees of at most 400 rows run on the host
        assert res[64][3]["host_splits"] == 0
        assert 0 < res[400][3]["host_splits"] < splits


def test_default_host_below_and_input_placement():
    x, mps, k, w, it = hc.cases()[hc.SAMPLED]
    want = hc.cpu(hc.SAMPLED)
    hc.same(rq.hierarchical_cluster(x, mps, k, w, it), want)
    xd = torch.from_numpy(x).cuda()
    for hb in (0, 64):
        got = rq.hierarchical_cluster(xd, mps, k, w, it, host_below=hb)
        hc.same(got, want)


def test_errors_are_returned():
    x = hc.cases()["identical_50_k4"][0]
    with pytest.raises(rq.RabitqError) as e:   # a size check on the host ends it: nothing loops
        rq.hierarchical_cluster(x, 20, 4, 0.0, 6)
    assert e.value.code == _abi.RBQ_INVALID_CONFIG and "single non-empty subcluster" in e.value.detail
    y = hc.cases()["crate_basic_100x8"][0].copy()
    y[3, 5] = np.inf
    for data in (y, torch.from_numpy(y).cuda()):
        with pytest.raises(rq.RabitqError) as e:
            rq.hierarchical_cluster(data, 20, 4, 1.0, 6)
        assert e.value.code == _abi.RBQ_INVALID_CONFIG and e.value.detail == "clustering input must be finite"
    z = hc.cases()["crate_basic_100x8"][0]
    for mps, k, it in ((20, 1, 5), (20, 0, 5), (20, 22, 5), (20, 4, 0)):
        with pytest.raises(rq.RabitqError) as e:
            rq.hierarchical_cluster(z, mps, k, 1.0, it)
        assert e.value.code == _abi.RBQ_INVALID_CONFIG
    with pytest.raises(rq.RabitqError):
        rq.hierarchical_cluster(np.zeros((0, 8), np.float32), 20, 4)


def _arrays(idx, D, ex, nlist):
    """Every array of the handle that rbq_debug_copy_index names (padded_dim D, ex_bits ex)."""
    Dc = (D + 63) // 64 * 64
    ln = idx.debug_copy_index("list_n", np.empty(nlist, np.uint32))
    nblocks = int(((ln + 31) // 32).sum())
    cpu_u = 128 // ex
    w4 = (D // 16 + cpu_u - 1) // cpu_u
    sizes = {"list_gb0": nlist * 4, "list_n": nlist * 4, "centroids": nlist * D * 4, "blocks": nblocks * (Dc * 4 + 384),
             "ids": nblocks * 32 * 8, "bsum": nblocks * 32, "delta": nblocks * 32 * 4, "vl": nblocks * 32 * 4,
             "cent_hi": nlist * D * 2, "cent_lo": nlist * D * 2, "cnorm2": nlist * 4, "ex": nblocks * 32 * w4 * 256,
             "fadd_ex": nblocks * 32 * 4, "fres_ex": nblocks * 32 * 4}
    return {name: idx.debug_copy_index(name, np.empty(nbytes, np.uint8)) for name, nbytes in sizes.items()}


def _exact_top(x, q, k, metric):
    if metric == "euclidean":
        d = ((q[:, None, :].astype(np.float64) - x[None].astype(np.float64)) ** 2).sum(-1)
    else:
        d = -(q.astype(np.float64) @ x.T.astype(np.float64))
    return np.argsort(d, axis=1, kind="stable")[:, :k]


@pytest.mark.parametrize("metric", ["euclidean", "angular"])
def test_mstg_index_fit_and_query(metric):
    rng = np.random.default_rng(11)
    x = rng.standard_normal((2000, 32)).astype(np.float32)
    q = rng.standard_normal((64, 32)).astype(np.float32)
    index = rq.MstgIndex(32, metric=metric, max_posting_size=64, rabitq_bits=7, max_iterations=8)
    with pytest.raises(RuntimeError):
        index.batch_query(q, 10)
    assert index.fit(x) is index and len(index) == 2000 and "2000 vectors" in repr(index)
    cent = rq.hierarchical_cluster_cpu(x, 64, 10, 1.0, 8)[0]
    assert np.array_equal(index.centroids.view(np.uint32), cent.view(np.uint32))
    m = rq.Metric.L2 if metric == "euclidean" else rq.Metric.InnerProduct
    want = rq.build_postings_on_device(x, cent, 7, m, 0.15, 8, True)
    a, b = _arrays(index.handle, 32, 6, len(cent)), _arrays(want, 32, 6, len(cent))
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    ids, dist, cnt = rq.mstg_search(index.handle, q, 10, 150, 0.6)
    res = index.batch_query(q, 10)
    assert len(res) == 64
    for i, r in enumerate(res):
        assert r.shape == (cnt[i], 2) and r.dtype == np.float32
        assert np.array_equal(r[:, 0], ids[i, :cnt[i]].astype(np.float32)) and np.array_equal(r[:, 1], dist[i, :cnt[i]])
    assert np.array_equal(index.query(q[5], 10), res[5])
    index.set_query_arguments(ef_search=20, pruning_epsilon=0.2)
    ids2, _, cnt2 = rq.mstg_search(index.handle, q, 10, 20, 0.2)
    r2 = index.batch_query(q, 10)
    assert all(np.array_equal(r2[i][:, 0], ids2[i, :cnt2[i]].astype(np.float32)) for i in range(64))
    top = _exact_top(x, q, 10, metric)
    recall = np.mean([len(set(top[i].tolist()) & set(ids[i, :cnt[i]].astype(np.int64).tolist())) / 10 for i in range(64)])
    print(f"recall@10 ({metric}, ef 150, eps 0.6, 64 queries): {recall:.3f}")  # recorded, not asserted: no reference number exists
