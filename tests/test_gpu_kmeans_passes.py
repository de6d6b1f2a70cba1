"""The k-means assignment in several passes (KmGemmAssign::run, km_common.hpp), which needs about 90 000 rows at k 256 to happen
by itself: rbq_debug_set_kmeans_chunk_rows caps the rows per pass at 128, so that the loop reuses its score, split-image and
shortlist buffers and offsets the norms, the assignments and the best distances by r0.  Every case equals the CPU restatement
bit for bit and the device run without the cap, stats included; rbq_debug_kmeans_assign_passes shows that the passes ran.
Then, without the cap, the magnitudes at which the shortlist gives up (squared norms from 1e37 on, up to +inf) and those whose
squared norms are f32 subnormals."""
import numpy as np
import pytest

import hcluster_cases as hc
import rabitq_rs_amd as rq
from conftest import make_dataset
from rabitq_rs_amd.index import lib
from rabitq_rs_amd.kmeans import KMeansConfig
from test_gpu_kmeans import _dups, _run_both, _same

pytestmark = pytest.mark.gpu

CAP = 128


def _ceil(a, b):
    return -(-a // b)


def _passes(n, k, cfg, rows_per_pass):
    """passes of one run: per restart, niter assignments of the training rows and one of every row"""
    kp = k * cfg.max_points_per_centroid
    train = max(min(n, kp), k)
    return cfg.nredo * (cfg.niter * _ceil(train, rows_per_pass) + _ceil(n, rows_per_pass))


def _counted(fn, cap):
    """fn() under a cap of `cap` rows per pass (0: none) -> (result, passes it took)"""
    L = lib()
    prev = L.rbq_debug_set_kmeans_chunk_rows(cap)
    try:
        p0 = L.rbq_debug_kmeans_assign_passes()
        out = fn()
        passes = L.rbq_debug_kmeans_assign_passes() - p0
    finally:
        L.rbq_debug_set_kmeans_chunk_rows(0)
    assert prev == 0  # (no earlier test left a cap behind)
    return out, passes


def _capped_equals_cpu_and_uncapped(data, k, cfg, torch_input=False):
    n = len(data)
    (gpu, st), passes = _counted(lambda: _run_both(data, k, cfg, torch_input=torch_input), CAP)
    assert passes == _passes(n, k, cfg, CAP), (passes, n, k, cfg)
    st0 = {}
    plain, passes0 = _counted(lambda: rq.run_kmeans_with_config(data, k, cfg, stats=st0), 0)
    assert passes0 == _passes(n, k, cfg, 1 << 40) == cfg.nredo * (cfg.niter + 1), passes0  # (these shapes fit one pass)
    _same(gpu, plain, "capped against uncapped")
    assert st == st0, (st, st0)  # shortlist_fallbacks, empty_reseeded, rng_draws, max_shortlist
    return gpu, st, passes


def test_the_knob_returns_the_previous_value_and_rounds_down_to_128():
    L = lib()
    try:
        assert L.rbq_debug_set_kmeans_chunk_rows(300) == 0
        assert L.rbq_debug_set_kmeans_chunk_rows(5) == 300
        data = make_dataset(700, 16, 4, 1)
        cfg = KMeansConfig(niter=2, seed=1)
        p0 = L.rbq_debug_kmeans_assign_passes()
        rq.run_kmeans_with_config(data, 8, cfg)
        assert L.rbq_debug_kmeans_assign_passes() - p0 == _passes(700, 8, cfg, 128) == 18  # 5 rows: the floor of 128
        assert L.rbq_debug_set_kmeans_chunk_rows(300) == 5
        p0 = L.rbq_debug_kmeans_assign_passes()
        rq.run_kmeans_with_config(data, 8, cfg)
        assert L.rbq_debug_kmeans_assign_passes() - p0 == _passes(700, 8, cfg, 256) == 9   # 300 rows: 256
        assert L.rbq_debug_set_kmeans_chunk_rows(0) == 300
    finally:
        L.rbq_debug_set_kmeans_chunk_rows(0)


@pytest.mark.parametrize("n", [129, 256, 257, 3000])
def test_pass_boundaries(n):
    """129: a second pass of one row behind 127 stale rows of the split image; 256: two full passes; 257: one row more"""
    data = make_dataset(n, 100, 8, 1000 + n)
    _, _, passes = _capped_equals_cpu_and_uncapped(data, 24, KMeansConfig(niter=8, seed=1))
    assert passes == 9 * _ceil(n, CAP)


def test_sampled_training_rows_and_all_rows_take_different_pass_counts():
    cfg = KMeansConfig(niter=8, seed=2, max_points_per_centroid=64)
    data = make_dataset(4000, 128, 10, 1000 + 4000 + 128)
    _, _, passes = _capped_equals_cpu_and_uncapped(data, 32, cfg)
    assert passes == 8 * 16 + 32  # 2048 training rows, 4000 rows


def test_reseed_candidates_across_pass_boundaries():
    """the candidate chunks (97 rows) do not line up with the passes (128 rows): a best distance written at the wrong offset
    changes the reseed candidates"""
    data = _dups(600, 128, 10, 11)
    _, st, _ = _capped_equals_cpu_and_uncapped(data, 24, KMeansConfig(niter=4, seed=12, decode_block_size=97))
    assert st["empty_reseeded"] > 0
    _, st, _ = _capped_equals_cpu_and_uncapped(data, 40, KMeansConfig(niter=3, seed=13, decode_block_size=97))
    assert st["empty_reseeded"] > 0  # (7 chunks x 8 candidates cover the empty clusters: no RNG draw)
    # one candidate chunk over all five passes: its 8 candidates run out and the RNG draws the rest
    _, st, _ = _capped_equals_cpu_and_uncapped(data, 40, KMeansConfig(niter=3, seed=13))
    assert st["empty_reseeded"] > 0 and st["rng_draws"] > 0


def test_spherical_and_restarts():
    data = make_dataset(2000, 100, 4, 3100, normalize=True)
    _capped_equals_cpu_and_uncapped(data, 12, KMeansConfig(niter=6, seed=6, spherical=True))
    data = make_dataset(1500, 128, 3, 2628)
    _, _, passes = _capped_equals_cpu_and_uncapped(data, 10, KMeansConfig(niter=4, nredo=3, seed=7))
    assert passes == 3 * 5 * 12


def test_fallback_rows_in_every_pass():
    # |x|^2 ~ 1.3e8 against distances ~ 1e2: every cluster lies within 2 eps, the shortlist (256) overflows for k = 300
    cfg = KMeansConfig(niter=3, seed=15)
    data = make_dataset(2000, 128, 12, 14) + np.float32(1000.0)
    _, st, _ = _capped_equals_cpu_and_uncapped(data, 300, cfg)
    assert st["shortlist_fallbacks"] == 4 * 2000, st  # every row of every assignment
    clean = make_dataset(2000, 128, 12, 14)
    _, st, _ = _capped_equals_cpu_and_uncapped(clean, 300, cfg)
    assert st["shortlist_fallbacks"] == 0 and 1 <= st["max_shortlist"] <= 256


def test_torch_device_input():
    data = make_dataset(1000, 100, 8, 77)
    _capped_equals_cpu_and_uncapped(data, 24, KMeansConfig(niter=5, seed=10), torch_input=True)


def test_hierarchical_clustering_above_256_subclusters():
    name = "gemm_3000x32_k300"
    x, mps, k, w, it = hc.cases()[name]
    want = hc.cpu(name)
    assert want[3]["splits"] == 1  # the root alone: `it` assignments of its 3000 rows and the final one
    got, passes = _counted(lambda: rq.hierarchical_cluster(x, mps, k, w, it, host_below=0), CAP)
    assert passes == (it + 1) * _ceil(3000, CAP)
    plain, passes0 = _counted(lambda: rq.hierarchical_cluster(x, mps, k, w, it, host_below=0), 0)
    assert passes0 == it + 1
    hc.same(got, want)
    hc.same(got, plain)
    for s in ("splits", "balance_moves", "empty_reseeded", "rng_draws", "host_splits"):
        assert got[3][s] == plain[3][s] and (s == "host_splits" or got[3][s] == want[3][s]), (s, got[3], plain[3], want[3])
    assert 0 < got[3]["arena_bytes"] < plain[3]["arena_bytes"]  # (the workspace of 128 rows per pass)


# ---- magnitudes (no cap) ------------------------------------------------------------------------------------------------
GIVE_UP = 1e37  # k_km_scan scores a row against every cluster when |x|^2 + max |c|^2 or its threshold is not below this


def _scaled(n, dim, scale):
    data = (make_dataset(n, dim, 6, 5).astype(np.float64) * scale).astype(np.float32)
    assert np.isfinite(data).all()
    return data


@pytest.mark.parametrize("scale", [1e-20, 1e-12, 3e17, 1e18, 3e18, 1e19])
@pytest.mark.parametrize("dim,k", [(16, 12), (128, 24)])
def test_magnitudes(dim, k, scale):
    """1e-20: the terms of the squared norms are f32 subnormals and the norms lie below the 2^-100 floor of eps, so every cluster is
    on every shortlist.  From 1e18
    on the squared norms pass 1e37 and the rows are scored against every cluster; at 1e19 they and every distance are +inf, no
    distance is below +inf and every row goes to cluster 0."""
    n, cfg = 1500, KMeansConfig(niter=4, seed=3)
    data = _scaled(n, dim, scale)
    gpu, st = _run_both(data, k, cfg)
    assert np.isfinite(gpu.centroids).all()
    norms = (data.astype(np.float64) ** 2).sum(axis=1)
    if scale == 1e-20:
        assert (data.astype(np.float64) ** 2).max() < 2.0 ** -126 and norms.max() < 2.0 ** -100  # (subnormal terms, sums below the floor)
        assert st["shortlist_fallbacks"] == 0 and st["max_shortlist"] == k
    if scale >= 1e18:
        assert st["shortlist_fallbacks"] > 0
    # a row whose own squared norm reaches the limit falls back in each of the niter + 1 assignments, whatever the centroids
    assert st["shortlist_fallbacks"] >= (cfg.niter + 1) * np.count_nonzero(norms >= 1.001 * GIVE_UP)
    if scale == 1e19:
        assert norms.min() > 1.001 * float(np.finfo(np.float32).max)
        assert st["shortlist_fallbacks"] == (cfg.niter + 1) * n
        assert np.all(gpu.assignments == 0)


@pytest.mark.parametrize("scale", [1e-20, 1e18])
def test_magnitudes_with_more_clusters_than_the_shortlist_holds(scale):
    """k 300: at 1e-20 all 300 clusters are within the eps floor, more than the 256 entries of a shortlist; at 1e18 the norm
    guard sends the rows to the same fallback"""
    n, cfg = 2000, KMeansConfig(niter=4, seed=3)
    data = _scaled(n, 32, scale)
    gpu, st = _run_both(data, 300, cfg)
    assert np.isfinite(gpu.centroids).all()
    norms = (data.astype(np.float64) ** 2).sum(axis=1)
    if scale == 1e-20:
        assert st["shortlist_fallbacks"] == (cfg.niter + 1) * n, st
    else:
        assert norms.min() >= 1.001 * GIVE_UP
        assert st["shortlist_fallbacks"] == (cfg.niter + 1) * n, st
