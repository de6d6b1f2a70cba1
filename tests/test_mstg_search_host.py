"""select_lists_cpu (rbq_build_mstg_select_lists, the CPU restatement of the MSTG search's list selection) against the NumPy
restatement tests/mstg_search_ref.py: lists and counts exactly.  No GPU."""
import numpy as np
import pytest

import rabitq_rs_amd as rq
from mstg_search_ref import NONE, select_lists_ref

EPSILONS = [-0.5, 0.0, 0.4, 0.6, 1e9, float("nan")]


def _same(q, c, ef, eps):
    lists, counts = rq.select_lists_cpu(q, c, ef, eps)
    rl, rc = select_lists_ref(q, c, ef, eps)
    assert lists.shape == rl.shape and lists.dtype == np.uint32
    assert np.array_equal(counts, rc), (counts, rc)
    assert np.array_equal(lists, rl)
    return lists, counts


def test_crate_centroid_search_inputs():
    # the inputs of hnsw.rs's test_centroid_search: the closest is centroid 0
    c = np.array([[0, 0], [10, 0], [0, 10], [10, 10]], np.float32)
    q = np.array([[0.1, 0.1]], np.float32)
    lists, counts = _same(q, c, 2, 1e9)
    assert counts[0] == 2 and lists[0, 0] == 0
    # centroids 1 and 2 are equally far: the lower index comes first
    assert lists[0, 1] == 1


@pytest.mark.parametrize("eps", EPSILONS)
@pytest.mark.parametrize("dim,k", [(16, 48), (20, 7), (128, 300), (3, 5)])
def test_seeded_data(dim, k, eps):
    rng = np.random.default_rng(dim * 1000 + k)
    c = rng.standard_normal((k, dim)).astype(np.float32)
    q = rng.standard_normal((24, dim)).astype(np.float32)
    for ef in (0, 1, 5, k, k + 9):
        _, counts = _same(q, c, ef, eps)
        if ef == 0 or np.isnan(eps):
            assert not counts.any()
        if eps == 1e9 and ef:
            assert (counts == min(ef, k)).all()


@pytest.mark.parametrize("eps", EPSILONS)
@pytest.mark.parametrize("k", [1, 2])
def test_one_and_two_lists(k, eps):
    rng = np.random.default_rng(k)
    c = rng.standard_normal((k, 32)).astype(np.float32)
    q = rng.standard_normal((9, 32)).astype(np.float32)
    for ef in (0, 1, k, k + 1, 150):
        _same(q, c, ef, eps)


@pytest.mark.parametrize("eps", EPSILONS)
def test_query_equal_to_a_centroid(eps):
    rng = np.random.default_rng(5)
    c = rng.standard_normal((40, 24)).astype(np.float32)
    q = c[[3, 17, 39]].copy()
    lists, counts = _same(q, c, 10, eps)
    if not np.isnan(eps):
        # d0 = 0: the threshold is 0 (or -0), and only lists at distance 0 stay
        assert (counts == 1).all() and lists[:, 0].tolist() == [3, 17, 39]


@pytest.mark.parametrize("eps", EPSILONS)
def test_duplicated_centroids(eps):
    rng = np.random.default_rng(6)
    base = rng.standard_normal((10, 16)).astype(np.float32)
    c = np.concatenate([base, base, base[:5]])  # ties at every rank, the cut at ef included
    q = rng.standard_normal((12, 16)).astype(np.float32)
    for ef in (1, 2, 3, 7, 25):
        lists, counts = _same(q, c, ef, eps)
        if eps == 1e9:
            assert (lists[:, 0] < 10).all()  # the lowest index of a tie group comes first


def test_threshold_equal_to_a_distance_bit_for_bit():
    # powers of two: d = 1, 2, 4, 8 exactly; 1 + eps = 2 and 4 make thr equal d of a centroid bit for bit (<= keeps it)
    c = np.zeros((4, 8), np.float32)
    c[:, 0] = [1, 2, 4, 8]
    q = np.zeros((1, 8), np.float32)
    for eps, want in ((1.0, 2), (3.0, 3), (0.999, 1), (7.0, 4)):
        lists, counts = _same(q, c, 4, eps)
        d = np.sqrt(((q - c) ** 2).sum(1, dtype=np.float32), dtype=np.float32)
        thr = np.float32(d[0] * (np.float32(1.0) + np.float32(eps)))
        assert counts[0] == want and (want == 1 or d[want - 1].view(np.uint32) == thr.view(np.uint32))


@pytest.mark.parametrize("eps", [0.6, float("nan")])
def test_nan_coordinate_selects_nothing(eps):
    rng = np.random.default_rng(8)
    c = rng.standard_normal((20, 16)).astype(np.float32)
    q = rng.standard_normal((3, 16)).astype(np.float32)
    q[1, 11] = np.nan
    lists, counts = _same(q, c, 5, eps)
    assert counts[1] == 0 and (lists[1] == NONE).all()
    c2 = c.copy()
    c2[19, 0] = np.nan  # one NaN distance anywhere: nothing for any query
    _, counts = _same(q, c2, 5, 0.6)
    assert not counts.any()


def test_infinite_closest_distance_selects_nothing():
    c = np.full((3, 8), 3e38, np.float32)
    q = np.full((1, 8), -3e38, np.float32)
    _, counts = _same(q, c, 3, 0.6)
    assert counts[0] == 0
