"""The device k-means (rbq_kmeans_device, k_kmeans.hip) against the CPU restatement rbq_build_kmeans_faiss, bit for bit:
centroids, assignments and objective; then IvfRabitqIndex.train end to end against train_with_clusters over the CPU
restatement's clustering, array for array, and its search results against the oracle."""
import ctypes as C

import numpy as np
import pytest

import rabitq_rs_amd as rq
from conftest import make_dataset
from rabitq_rs_amd.kmeans import KMeansConfig, first_draw
from test_gpu_encode_optimal import _same_index
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu


def _same(gpu, cpu, what=""):
    assert np.array_equal(gpu.assignments, cpu.assignments), f"{what}: {np.count_nonzero(gpu.assignments != cpu.assignments)} assignments differ"
    bad = np.nonzero((gpu.centroids.view(np.uint32) != cpu.centroids.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, f"{what}: centroids {bad[:8]} differ"
    assert np.float64(gpu.objective).view(np.uint64) == np.float64(cpu.objective).view(np.uint64), (what, gpu.objective, cpu.objective)


def _run_both(data, k, cfg, torch_input=False):
    cst, gst = {}, {}
    cpu = rq.builder.run_kmeans_with_config_cpu(data, k, cfg, stats=cst)
    if torch_input:
        import torch
        data = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    gpu = rq.run_kmeans_with_config(data, k, cfg, stats=gst)
    _same(gpu, cpu, repr(cfg))
    assert gst["empty_reseeded"] == cst["empty_reseeded"] and gst["rng_draws"] == cst["rng_draws"]
    return gpu, gst


def _dups(n, dim, distinct, seed):
    r = np.random.default_rng(seed)
    base = r.normal(size=(distinct, dim)).astype(np.float32)
    return base[r.integers(0, distinct, n)]


@pytest.mark.parametrize("n,dim,k,cfg", [
    pytest.param(3000, 100, 24, KMeansConfig(niter=8, seed=1), id="d100_all_rows"),
    pytest.param(4000, 128, 32, KMeansConfig(niter=8, seed=2, max_points_per_centroid=64), id="d128_sampled"),
    pytest.param(3000, 960, 40, KMeansConfig(niter=6, seed=3), id="d960_all_rows"),
    pytest.param(5000, 960, 16, KMeansConfig(niter=5, seed=4, max_points_per_centroid=200), id="d960_sampled"),
    pytest.param(2500, 128, 20, KMeansConfig(niter=6, seed=5, decode_block_size=300), id="d128_chunks"),
    pytest.param(2000, 100, 12, KMeansConfig(niter=6, seed=6, spherical=True), id="d100_spherical"),
    pytest.param(1500, 128, 10, KMeansConfig(niter=4, nredo=3, seed=7), id="d128_nredo3"),
    pytest.param(800, 960, 1, KMeansConfig(niter=3, seed=8), id="d960_k1"),
    pytest.param(300, 100, 300, KMeansConfig(niter=3, seed=9), id="d100_k_eq_n"),
])
def test_device_kmeans_matches_cpu_restatement(n, dim, k, cfg):
    data = make_dataset(n, dim, max(k // 3, 1), 1000 + n + dim, normalize=cfg.spherical)
    _run_both(data, k, cfg)


def test_torch_input_matches_numpy_input():
    data = make_dataset(3000, 960, 10, 77)
    g1, _ = _run_both(data, 24, KMeansConfig(niter=5, seed=10), torch_input=True)
    g2 = rq.run_kmeans_with_config(data, 24, KMeansConfig(niter=5, seed=10))
    _same(g1, g2)


def test_empty_clusters_reseed_from_candidates_and_rng():
    data = _dups(600, 128, 10, 11)
    _, st = _run_both(data, 24, KMeansConfig(niter=4, seed=12, decode_block_size=97))
    assert st["empty_reseeded"] > 0
    _, st = _run_both(data, 40, KMeansConfig(niter=3, seed=13))
    assert st["rng_draws"] > 0


def test_large_offset_forces_counted_fallbacks():
    # |x|^2 ~ 1.3e8 against distances ~ 1e2: every cluster lies within 2 eps, the shortlist (256) overflows for k = 300
    data = make_dataset(2000, 128, 12, 14) + np.float32(1000.0)
    _, st = _run_both(data, 300, KMeansConfig(niter=3, seed=15))
    assert st["shortlist_fallbacks"] > 0
    clean = make_dataset(2000, 128, 12, 14)
    _, st = _run_both(clean, 300, KMeansConfig(niter=3, seed=15))
    assert st["shortlist_fallbacks"] == 0 and 1 <= st["max_shortlist"] <= 256


def test_two_runs_identical_bytes():
    data = make_dataset(6000, 960, 20, 16)
    cfg = KMeansConfig(niter=6, seed=17)
    a = rq.run_kmeans_with_config(data, 64, cfg)
    b = rq.run_kmeans_with_config(data, 64, cfg)
    assert a.centroids.tobytes() == b.centroids.tobytes() and a.assignments.tobytes() == b.assignments.tobytes()
    assert np.float64(a.objective).tobytes() == np.float64(b.objective).tobytes()


def test_rejections_on_the_device_path():
    import torch
    data = make_dataset(50, 16, 3, 18)
    for k, cfg, msg in ((0, KMeansConfig(), "k must be positive"), (51, KMeansConfig(), "k cannot exceed number of samples"),
                        (3, KMeansConfig(niter=0), "max_iter must be positive"), (3, KMeansConfig(nredo=0), "nredo must be positive"),
                        (3, KMeansConfig(decode_block_size=0), "decode_block_size must be positive")):
        with pytest.raises(rq.RabitqError) as e:
            rq.run_kmeans_with_config(data, k, cfg)
        assert e.value.kind == "InvalidConfig" and e.value.detail == msg
    # the library's own check of device data (no Python validation in front)
    bad = data.copy()
    bad[10, 3] = np.nan
    x = torch.from_numpy(bad).cuda()
    asg = torch.empty(50, dtype=torch.int32, device="cuda")
    cent, obj = np.empty((3, 16), np.float32), C.c_double()
    L = rq.index.lib()
    rc = L.rbq_kmeans_device(C.c_void_p(x.data_ptr()), 50, 16, 3, 2, 1, 1, 0, 256, 32768, 0, cent.ctypes.data,
                             C.c_void_p(asg.data_ptr()), C.byref(obj), None)
    assert rc == rq._abi.RBQ_INVALID_CONFIG and rq.index._detail() == "k-means input must be finite"
    rc = L.rbq_kmeans_device(C.c_void_p(x.data_ptr()), 0, 16, 3, 2, 1, 1, 0, 256, 32768, 0, cent.ctypes.data,
                             C.c_void_p(asg.data_ptr()), C.byref(obj), None)
    assert rc == rq._abi.RBQ_INVALID_CONFIG and rq.index._detail() == "k-means requires non-empty data"


# ---- IvfRabitqIndex.train ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("faster", [False, True])
@pytest.mark.parametrize("metric", [0, 1])
def test_train_matches_train_with_clusters_over_cpu_kmeans(metric, faster):
    n, dim, nlist, bits, seed = 4000, 200, 32, 7, 19
    data = make_dataset(n, dim, 8, 20, normalize=(metric == 1))
    cfg = KMeansConfig(niter=30, seed=first_draw(seed ^ 0x5A5A5A5A5A5A5A5A))
    km = rq.builder.run_kmeans_with_config_cpu(data, nlist, cfg)
    built = rq.builder.train_with_clusters(data, km.centroids, km.assignments, bits, metric, 1, seed, faster)
    ref = rq.IvfRabitqIndex.from_built(built)
    idx = rq.IvfRabitqIndex.train(data, nlist, bits, metric, rq.RotatorType.FhtKacRotator, seed, faster)
    _same_index(ref, idx, built.hdr, nlist)
    q = make_dataset(32, dim, 8, 21, normalize=(metric == 1))
    _compare(built, idx, q, 10, 8)
    ref.close(); idx.close()


def test_train_rejects_like_the_crate():
    data = make_dataset(20, 8, 2, 22)
    for args, msg in (((data[:0], 4, 7), "training data must be non-empty"), ((data, 0, 7), "nlist must be positive"),
                      ((data, 4, 0), "total_bits must be between 1 and 16"), ((data, 4, 17), "total_bits must be between 1 and 16"),
                      ((data, 21, 7), "nlist cannot exceed number of vectors")):
        with pytest.raises(rq.RabitqError) as e:
            rq.IvfRabitqIndex.train(*args, 0, 1, 1, True)
        assert e.value.kind == "InvalidConfig" and e.value.detail == msg


def test_large_50k_d960_k256_niter30_matches_cpu():
    rng = np.random.default_rng(23)
    data = make_dataset(50000, 960, 64, 24)
    data += 0.05 * rng.standard_normal(data.shape, dtype=np.float32)
    _, st = _run_both(data, 256, KMeansConfig(niter=30, seed=25))
    assert st["max_shortlist"] >= 1
