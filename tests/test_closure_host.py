"""MSTG closure assignment on the CPU: the builder's restatement (rbq_build_closure_assign, OpenMP) equals the independent NumPy
restatement of the crate's text (tests/closure_ref.py) exactly, in lists, order and counts; and the argument checks of the device
entry points (include/rbq_mstg.h) that return before any HIP call.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import closure_cases as cc
import closure_ref
import rabitq_rs_amd as rq
from rabitq_rs_amd import _abi, index as ix, mstg


def _same(x, c, eps, m):
    want_l, want_n = closure_ref.closure_assign(x, c, eps, m)
    got_l, got_n = rq.closure_assign_cpu(x, c, eps, m)
    assert np.array_equal(got_n, want_n)
    assert np.array_equal(got_l, want_l)
    assert (got_n >= 1).all() and (got_l[:, 0] != mstg.NONE).all()


@pytest.mark.parametrize("case", range(len(cc.CRATE_UNIT)))
def test_the_crates_own_unit_test_inputs(case):
    eps, m, v, c = cc.CRATE_UNIT[case]
    v, c = np.asarray(v, np.float32), np.asarray(c, np.float32)
    _same(v, c, eps, m)
    lists, counts = rq.closure_assign_cpu(v, c, eps, m)
    rows = [list(lists[i, :counts[i]]) for i in range(len(v))]
    if case == 0:
        assert rows == [[0]]
    elif case == 1:
        assert rows[0][0] == 0 and (0 in rows[1] or 1 in rows[1])
    elif case == 2:
        assert len(rows[0]) <= 3 and (0 in rows[0] or 1 in rows[0])
    else:
        assert len(rows[0]) <= 3


def test_main_case_is_not_degenerate_and_matches():
    """A condition on the input, from closure_ref's output alone: mean replication >= 1.2, and the RNG rule removes a candidate
    for at least 5 % of the vectors.  Then parity on it."""
    x, c, eps, m = cc.main_case()
    st = {}
    want_l, want_n = closure_ref.closure_assign(x, c, eps, m, st)
    print("replication", want_n.mean(), "rng-rule rows", (st["removed"] > 0).mean())
    assert want_n.mean() >= 1.2
    assert (st["removed"] > 0).mean() >= 0.05
    got_l, got_n = rq.closure_assign_cpu(x, c, eps, m)
    assert np.array_equal(got_n, want_n) and np.array_equal(got_l, want_l)


def test_default_epsilon_case_is_not_degenerate_and_matches():
    """The crate's default configuration on data chosen to replicate within epsilon 0.15: replication >= 1.1 and the RNG rule
    at work on at least 5 % of the vectors, from closure_ref's output alone."""
    x, c, eps, m = cc.default_epsilon_case()
    st = {}
    want_l, want_n = closure_ref.closure_assign(x, c, eps, m, st)
    print("replication", want_n.mean(), "rng-rule rows", (st["removed"] > 0).mean())
    assert want_n.mean() >= 1.1
    assert (st["removed"] > 0).mean() >= 0.05
    got_l, got_n = rq.closure_assign_cpu(x, c, eps, m)
    assert np.array_equal(got_n, want_n) and np.array_equal(got_l, want_l)


@pytest.mark.parametrize("name", sorted(cc.shortlist_dim_cases()))
def test_many_centroids_at_odd_dims(name):
    x, c = cc.shortlist_dim_cases()[name]
    for eps, m in ((0.15, 8), (2.0, 16), (10.0, 3)):
        _same(x, c, eps, m)


@pytest.mark.parametrize("name", sorted(cc.dim_cases()))
@pytest.mark.parametrize("eps", cc.EPSILONS)
def test_dims_and_list_counts(name, eps):
    x, c = cc.dim_cases()[name]
    for m in cc.REPLICAS:
        _same(x, c, eps, m)


@pytest.mark.parametrize("name", sorted(cc.tie_cases()))
@pytest.mark.parametrize("eps", cc.EPSILONS)
def test_ties(name, eps):
    x, c = cc.tie_cases()[name]
    for m in cc.REPLICAS:
        _same(x, c, eps, m)


def test_ties_keep_ascending_centroid_index():
    x, c = cc.tie_cases()["duplicated_centroids"]
    st = {}
    closure_ref.closure_assign(x, c, 10.0, 16, st)
    k0 = 10
    dup = {k0 + i: 2 * i for i in range(5)}
    dup.update({k0 + 5 + i: i for i in range(3)})
    seen = 0
    for order in st["order"]:
        for late, early in dup.items():
            if late in order and early in order:
                assert order.index(early) < order.index(late)
                seen += 1
    assert seen > 100


def test_cpu_restatement_rejects_what_the_crate_panics_on():
    x, c = np.zeros((2, 4), np.float32), np.zeros((3, 4), np.float32)
    for eps, m in ((0.15, 0), (-0.1, 8), (float("nan"), 8), (float("inf"), 8)):
        with pytest.raises(rq.RabitqError) as e:
            rq.closure_assign_cpu(x, c, eps, m)
        assert e.value.code == _abi.RBQ_INVALID_CONFIG
    for xx, cc_ in ((np.zeros((0, 4), np.float32), c), (x, np.zeros((0, 4), np.float32))):
        with pytest.raises(rq.RabitqError):
            rq.closure_assign_cpu(xx, cc_, 0.15, 8)
    with pytest.raises(rq.RabitqError) as e:
        rq.closure_assign_cpu(x, np.zeros((3, 5), np.float32), 0.15, 8)
    assert e.value.code == _abi.RBQ_DIMENSION_MISMATCH


def _closure_rc(cent, k, dim, data, n, eps, m, out=True):
    lists, counts = np.zeros((max(n, 1), max(m, 1)), np.uint32), np.zeros(max(n, 1), np.uint32)
    rc = ix.lib().rbq_mstg_closure_assign(cent, k, dim, data, n, eps, m, 0, 0, lists.ctypes.data if out else None, counts.ctypes.data)
    return rc, ix._detail()


def test_device_closure_checks_its_arguments_before_any_hip_call():
    x, c = np.zeros((2, 4), np.float32), np.zeros((3, 4), np.float32)
    xp, cp = x.ctypes.data, c.ctypes.data
    assert _closure_rc(cp, 3, 4, xp, 2, 0.15, 0) == (_abi.RBQ_INVALID_CONFIG, "max_replicas must be positive")
    assert _closure_rc(cp, 3, 4, xp, 2, 0.15, 65) == (_abi.RBQ_INVALID_CONFIG, "max_replicas above 64 is not supported")
    for eps in (-0.5, float("nan"), float("inf")):
        assert _closure_rc(cp, 3, 4, xp, 2, eps, 8) == (_abi.RBQ_INVALID_CONFIG, "closure epsilon must be finite and not negative")
    assert _closure_rc(cp, 3, 4, xp, 0, 0.15, 8) == (_abi.RBQ_INVALID_CONFIG, "no vectors")
    assert _closure_rc(cp, 0, 4, xp, 2, 0.15, 8) == (_abi.RBQ_INVALID_CONFIG, "nlist must be positive")
    assert _closure_rc(cp, 3, 0, xp, 2, 0.15, 8) == (_abi.RBQ_INVALID_CONFIG, "dimension must be positive")
    assert _closure_rc(None, 3, 4, xp, 2, 0.15, 8) == (_abi.RBQ_INVALID_CONFIG, "null buffer")
    assert _closure_rc(cp, 3, 4, None, 2, 0.15, 8) == (_abi.RBQ_INVALID_CONFIG, "null buffer")
    assert _closure_rc(cp, 3, 4, xp, 2, 0.15, 8, out=False) == (_abi.RBQ_INVALID_CONFIG, "null buffer")
    sl, sl_n = np.zeros((2, 256), np.uint32), np.zeros(2, np.uint32)
    assert ix.lib().rbq_mstg_debug_closure_shortlist(cp, 3, 4, xp, 2, 0, 0, 0, sl.ctypes.data, sl_n.ctypes.data) == _abi.RBQ_INVALID_CONFIG
    assert isinstance(mstg.closure_fallbacks(), int)


def _build_rc(hdr, cent, data, n, eps=0.15, m=8, rescale=_abi.RESCALE_MODES["const"], t=1.0, out=True):
    h = C.c_void_p()
    rc = ix.lib().rbq_mstg_build_device(hdr, cent, data, n, eps, m, rescale, t, 0, 0, C.byref(h) if out else None)
    assert not h.value
    return rc, ix._detail()


def test_device_build_checks_its_arguments_before_any_hip_call():
    c = np.random.default_rng(1).standard_normal((3, 16)).astype(np.float32)
    x = np.random.default_rng(2).standard_normal((5, 16)).astype(np.float32)
    none = rq.builder.train_with_clusters(c, c, np.arange(3, dtype=np.uint32), 7, 0, rq.RotatorType.NoRotation, 42, True)
    c64 = np.random.default_rng(3).standard_normal((3, 64)).astype(np.float32)
    fht = rq.builder.train_with_clusters(c64, c64, np.arange(3, dtype=np.uint32), 7, 0, rq.RotatorType.FhtKacRotator, 42, True)
    hp, xp, cp = ix._addr(none.hdr_ptr), x.ctypes.data, c.ctypes.data
    assert _build_rc(None, cp, xp, 5) == (_abi.RBQ_INVALID_CONFIG, "null header")
    assert _build_rc(ix._addr(fht.hdr_ptr), cp, xp, 5) == (_abi.RBQ_INVALID_CONFIG, "MSTG posting lists take rotator RBQ_ROTATOR_NONE")
    assert _build_rc(hp, None, xp, 5) == (_abi.RBQ_INVALID_CONFIG, "null buffer")
    assert _build_rc(hp, cp, None, 5) == (_abi.RBQ_INVALID_CONFIG, "null buffer")
    assert _build_rc(hp, cp, xp, 0) == (_abi.RBQ_INVALID_CONFIG, "no vectors")
    assert _build_rc(hp, cp, xp, 5, m=0) == (_abi.RBQ_INVALID_CONFIG, "max_replicas must be positive")
    assert _build_rc(hp, cp, xp, 5, eps=-1.0) == (_abi.RBQ_INVALID_CONFIG, "closure epsilon must be finite and not negative")
    assert _build_rc(hp, cp, xp, 5, eps=float("nan"))[0] == _abi.RBQ_INVALID_CONFIG
    assert _build_rc(hp, cp, xp, 5, rescale=7)[0] == _abi.RBQ_INVALID_CONFIG
    assert _build_rc(hp, cp, xp, 5, t=0.0) == (_abi.RBQ_INVALID_CONFIG, "the device encoder needs the constant rescale factor (faster config)")
    assert _build_rc(hp, cp, xp, 5, out=False) == (_abi.RBQ_INVALID_CONFIG, "null out pointer")
    none.close()
    fht.close()
