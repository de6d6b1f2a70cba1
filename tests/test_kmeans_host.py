"""The CPU restatement of run_kmeans_with_config (rbq_build_kmeans_faiss) against the numpy restatement of
tests/kmeans_ref.py, bit for bit: centroids, assignments and objective.  No GPU."""
import numpy as np
import pytest

import rabitq_rs_amd as rq
from rabitq_rs_amd.kmeans import KMeansConfig

import kmeans_ref


def _same(res, ref):
    cent, asg, obj, _ = ref
    assert res.centroids.dtype == np.float32 and res.assignments.dtype == np.uint32
    assert np.array_equal(res.centroids.view(np.uint32), cent.view(np.uint32))
    assert np.array_equal(res.assignments, asg)
    assert res.objective == obj  # same f64 bits


def _check(data, k, **cfg):
    st = {}
    res = rq.builder.run_kmeans_with_config_cpu(data, k, KMeansConfig(**cfg), stats=st)
    ref = kmeans_ref.run_kmeans(data, k, **cfg)
    _same(res, ref)
    assert st == ref[3]
    return res, st


def _blobs(n, dim, centers, seed, spread=0.3):
    r = np.random.default_rng(seed)
    c = r.normal(size=(centers, dim)).astype(np.float32) * 4
    return (c[r.integers(0, centers, n)] + spread * r.normal(size=(n, dim))).astype(np.float32)


def test_all_rows_trained():
    _check(_blobs(600, 20, 8, 1), 8, niter=6, seed=5)


def test_sampled_run():
    data = _blobs(700, 12, 5, 2)  # 700 > 2 * 256: a shuffled, sorted sample of 512 rows
    res, _ = _check(data, 2, niter=5, seed=11)
    assert res.assignments.shape == (700,)


def test_small_max_points_per_centroid_and_chunks():
    _check(_blobs(500, 9, 6, 3), 6, niter=5, seed=3, max_points_per_centroid=40, decode_block_size=37)


def test_several_chunks():
    _check(_blobs(400, 16, 10, 4), 10, niter=4, seed=9, decode_block_size=50)


def test_empty_clusters_reseed_from_candidates_and_rng():
    # 6 distinct points repeated: k = 12 leaves clusters empty in every iteration; a chunk of 3 rows gives few candidates
    r = np.random.default_rng(5)
    base = r.normal(size=(6, 7)).astype(np.float32)
    data = base[r.integers(0, 6, 60)]
    _, st = _check(data, 12, niter=4, seed=21, decode_block_size=3)
    assert st["empty_reseeded"] > 0
    # one chunk, all distances 0 after the first iteration: 8 candidates, then the RNG
    _, st = _check(data, 20, niter=3, seed=22)
    assert st["rng_draws"] > 0 and st["empty_reseeded"] > st["rng_draws"]


def test_spherical():
    _check(_blobs(300, 10, 4, 6), 4, niter=5, seed=7, spherical=True)


def test_nredo_three():
    _check(_blobs(300, 8, 5, 7, spread=1.5), 5, niter=3, nredo=3, seed=13)


def test_k_one_and_k_n():
    data = _blobs(50, 6, 3, 8)
    _check(data, 1, niter=3, seed=1)
    _check(data, 50, niter=3, seed=2)


def test_defaults_match_the_crate():
    c = KMeansConfig()
    assert (c.niter, c.nredo, c.seed, c.spherical, c.max_points_per_centroid, c.decode_block_size) == (25, 1, 42, False, 256, 32768)


@pytest.mark.parametrize("case, msg", [
    ("empty", "k-means requires non-empty data"),
    ("k0", "k must be positive"),
    ("niter0", "max_iter must be positive"),
    ("k_gt_n", "k cannot exceed number of samples"),
    ("nredo0", "nredo must be positive"),
    ("dbs0", "decode_block_size must be positive"),
    ("nan", "k-means input must be finite"),
    ("inf", "k-means input must be finite"),
])
def test_rejected_configurations(case, msg):
    data = _blobs(20, 4, 2, 9)
    k, cfg = 3, KMeansConfig(niter=2)
    if case == "empty":
        data = data[:0]
    elif case == "k0":
        k = 0
    elif case == "niter0":
        cfg.niter = 0
    elif case == "k_gt_n":
        k = 21
    elif case == "nredo0":
        cfg.nredo = 0
    elif case == "dbs0":
        cfg.decode_block_size = 0
    elif case == "nan":
        data[3, 2] = np.nan
    else:
        data[7, 0] = np.inf
    with pytest.raises(rq.RabitqError) as e:
        rq.builder.run_kmeans_with_config_cpu(data, k, cfg)
    assert e.value.kind == "InvalidConfig" and e.value.detail == msg


def test_library_rejects_directly():
    # the C entry point checks on its own (no Python validation in front of it)
    import ctypes as C
    L = rq.builder.lib()
    data = _blobs(10, 3, 2, 10)
    data[2, 1] = np.inf
    cent, asg, obj = np.empty((2, 3), np.float32), np.empty(10, np.uint32), C.c_double()
    args = (cent.ctypes.data, asg.ctypes.data, C.byref(obj), None)
    assert L.rbq_build_kmeans_faiss(data.ctypes.data, 10, 3, 2, 2, 1, 1, 0, 256, 32768, *args) == rq._abi.RBQ_INVALID_CONFIG
    data[2, 1] = 0
    for n, k, it, redo, dbs in ((10, 0, 2, 1, 8), (10, 11, 2, 1, 8), (10, 2, 0, 1, 8), (10, 2, 2, 0, 8), (10, 2, 2, 1, 0)):
        assert L.rbq_build_kmeans_faiss(data.ctypes.data, n, 3, k, it, redo, 1, 0, 256, dbs, *args) == rq._abi.RBQ_INVALID_CONFIG
    assert L.rbq_build_kmeans_faiss(data.ctypes.data, 10, 3, 2, 2, 1, 1, 0, 256, 8, *args) == rq._abi.RBQ_OK


def test_train_rejects_before_any_device_work():
    """IvfRabitqIndex.train's checks (src/ivf.rs:957-983) fire on the host, in the crate's order and with its messages."""
    data = _blobs(20, 8, 2, 11)
    for args, msg in (((data[:0], 4, 7), "training data must be non-empty"), ((data, 0, 7), "nlist must be positive"),
                      ((data, 4, 0), "total_bits must be between 1 and 16"), ((data, 4, 17), "total_bits must be between 1 and 16"),
                      ((data[0], 4, 7), "input vectors must share the same dimension"),
                      ((data, 21, 7), "nlist cannot exceed number of vectors")):
        with pytest.raises(rq.RabitqError) as e:
            rq.IvfRabitqIndex.train(*args, 0, 1, 1, True)
        assert e.value.kind == "InvalidConfig" and e.value.detail == msg


def test_train_kmeans_seed_is_first_draw():
    # rng.next_u64() of StdRng::seed_from_u64(seed ^ 0x5a5a...) in the crate: the first output of the project's Rng
    for seed in (0, 42, 2**64 - 1):
        assert rq.kmeans.first_draw(seed ^ 0x5A5A5A5A5A5A5A5A) == kmeans_ref.Rng(seed ^ 0x5A5A5A5A5A5A5A5A).next()
