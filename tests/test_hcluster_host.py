"""MSTG hierarchical balanced clustering on the CPU: the builder's restatement (rbq_build_hcluster) equals the independent NumPy
restatement of the crate's text (tests/hcluster_ref.py) in every array, keeps the crate's invariants and refuses what the crate
panics or never ends on.  No GPU."""
import numpy as np
import pytest

import hcluster_cases as hc
import hcluster_ref
import rabitq_rs_amd as rq
from rabitq_rs_amd import _abi

STAT_KEYS = ("splits", "balance_moves", "empty_reseeded", "rng_draws")


@pytest.mark.parametrize("name", sorted(hc.cases()))
def test_equals_the_numpy_restatement(name):
    x, mps, k, w, it = hc.cases()[name]
    want = hcluster_ref.cluster(x, mps, k, w, it)
    got = hc.cpu(name)
    hc.same(got, want)
    assert {s: got[3][s] for s in STAT_KEYS} == want[3]
    assert got[3]["host_splits"] == 0


@pytest.mark.parametrize("name", sorted(hc.cases()))
def test_invariants(name):
    x, mps, k, w, it = hc.cases()[name]
    cent, off, mem, st = hc.cpu(name)
    assert np.array_equal(np.sort(mem), np.arange(len(x), dtype=np.uint32))
    sizes = np.diff(off.astype(np.int64))
    assert off[0] == 0 and off[-1] == len(x) and (sizes > 0).all() and (sizes <= mps).all()
    for c in range(len(sizes)):
        s = np.zeros(x.shape[1], np.float32)
        for r in mem[off[c]:off[c + 1]]:
            s = s + x[r]
        assert np.array_equal((s / np.float32(sizes[c])).view(np.uint32), cent[c].view(np.uint32))


def test_the_crates_unit_shapes_hold_its_assertions():
    _, off, _, _ = hc.cpu("crate_basic_100x8")
    sizes = np.diff(off.astype(np.int64))
    assert (sizes <= 20).all() and sizes.sum() == 100
    _, off, _, _ = hc.cpu("crate_balance_1000x32")
    sizes = np.diff(off.astype(np.int64)).astype(np.float32)
    cov = np.sqrt(((sizes - sizes.mean()) ** 2).mean()) / sizes.mean()
    print("mean cluster size", sizes.mean(), "CoV", cov)
    assert cov < 0.6 and (sizes > 0).all()


def test_the_cases_reach_their_paths():
    assert hc.cpu(hc.BALANCING)[3]["balance_moves"] > 0
    for name in hc.IDENTICAL:
        assert hc.cpu(name)[3]["empty_reseeded"] > 0 and hc.cpu(name)[3]["balance_moves"] > 0
    assert hc.cpu("identical_60_k12")[3]["rng_draws"] > 0
    assert hc.cpu(hc.SAMPLED)[3]["splits"] > 1


def test_balance_weight_edges():
    x, mps, k, _, it = hc.cases()[hc.BALANCING]
    off_nan = rq.hierarchical_cluster_cpu(x, mps, k, float("nan"), it)
    off_zero = rq.hierarchical_cluster_cpu(x, mps, k, 0.0, it)
    off_neg = rq.hierarchical_cluster_cpu(x, mps, k, -1.0, it)
    hc.same(off_nan, off_zero)
    hc.same(off_neg, off_zero)
    assert off_zero[3]["balance_moves"] == 0
    inf = rq.hierarchical_cluster_cpu(x, mps, k, float("inf"), it)
    assert inf[3]["balance_moves"] == 0  # max_allowed saturates: nothing is ever oversized
    hc.same(inf, off_zero)
    hc.same(rq.hierarchical_cluster_cpu(x, mps, k, float("inf"), it), hcluster_ref.cluster(x, mps, k, float("inf"), it))


def _refused(x, mps, k, w=1.0, it=5):
    with pytest.raises(rq.RabitqError) as e:
        rq.hierarchical_cluster_cpu(x, mps, k, w, it)
    assert e.value.code == _abi.RBQ_INVALID_CONFIG
    return e.value.detail


def test_errors():
    x = np.random.default_rng(1).random((40, 4), dtype=np.float32)
    assert _refused(np.zeros((0, 4), np.float32), 10, 4) in ("no vectors", "null buffer")
    assert _refused(np.zeros((4, 0), np.float32), 10, 4) in ("dimension must be positive", "null buffer")
    assert _refused(x, 10, 4, it=0) == "max_iterations must be positive"
    assert _refused(x, 10, 0) == "branching_factor must be at least 2"
    assert _refused(x, 10, 1) == "branching_factor must be at least 2"
    assert "max_posting_size + 1" in _refused(x, 10, 12)
    rq.hierarchical_cluster_cpu(x, 10, 11, 1.0, 3)  # k == max_posting_size + 1 is served
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[17, 2] = bad
        assert _refused(y, 10, 4) == "clustering input must be finite"


def test_identical_rows_without_balancing_are_refused_not_looped_on():
    x = hc.cases()["identical_50_k4"][0]
    for w in (0.0, -1.0, float("nan")):
        assert "single non-empty subcluster" in _refused(x, 20, 4, w)
    with pytest.raises(hcluster_ref.Stuck):
        hcluster_ref.cluster(x, 20, 4, 0.0, 5)
