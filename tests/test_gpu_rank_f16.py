"""The one-product f16 ranking GEMM (k_rank_f16_db; rank_mfma.hpp header, "ONE f16 PRODUCT") on the GPU.

Forced route (option rank_f16 = 1), every case:
  (a) the images ("cent_f16", "rot_f16") equal the numpy restatement (tests/rank_f16_bound.py) bit for bit; the residuals
      ("cent_f16_resid", "rank_resid") are at or above their float64 value and within 1e-5 relative of it;
  (b) every score is inside the GEMM's float64 budget;
  (c) on a sample, |A - canonical| <= eps, eps as k_select_mfma evaluates it on this route;
  (d) no rank fallback;
  (e) for one shape per tile and metric, ids, counts and scores equal the oracle's.
Shapes: D 64 (one slab of 64), 192 (three) and 960 (fifteen); 129 and 1000 lists, 1 / 127 / 129 / 1025 queries: ragged tile edges in
both directions and clamped rows in every tile of 64, 128 and 128 x 256.  The three kernels that write the query image are all
reached (test_gpu_rank_lines._prep_opts).
By rule (default options): D 256, 3072 lists, 1024 queries — 192 tiles of 128 x 128, the smallest big call — takes the route; the
same call with rank_f16 = 0 runs split-bf16 and returns the same bits.
Gate and fallback: centroids that flush (data x 1e-4) or overflow (x 1e5) keep the index on split-bf16; queries x 1e6 have an image
that is not finite and fall back; queries x 100 stay inside the budget.  Each ends in the oracle's results.
Run with -s to see the worst error / budget per case."""
import numpy as np
import pytest

import rank_bound as rb
import rank_f16_bound as fb
import test_gpu_rank_bound as trb
from conftest import make_dataset
from test_gpu_parity import RTOL, _compare
from test_gpu_rank_bound import TOP_K, _Case, _device_search, _queries, _rank_workgroups, _set, _tiles
from test_gpu_rank_lines import _prep_opts

pytestmark = pytest.mark.gpu

DIMS = [64, 192, 960]
NLISTS = [129, 1000]
NQS = [1, 127, 129, 1025]
TILES = [64, 128, 256]
NPROBE = 16


def _data_with_1e5(orig):
    def data(kind, n, dim, seed):
        if kind == "mix_1e5":
            return (make_dataset(n, dim, 16, seed) * np.float32(1e5)).astype(np.float32)
        return orig(kind, n, dim, seed)
    return data


@pytest.fixture(scope="module")
def env():
    import torch
    cache = {}
    stream = torch.cuda.Stream(torch.device("cuda", 0))

    def get(dim, nlist, metric, kind="mix"):
        k = (dim, nlist, metric, kind)
        if k not in cache:
            with pytest.MonkeyPatch.context() as mp:  # (one more magnitude than test_gpu_rank_bound's kinds)
                mp.setattr(trb, "_data", _data_with_1e5(trb._data))
                case = _Case(dim, nlist, metric, 1, kind)
            assert case.D == dim
            # (a), centroid side
            case.cbits = case.idx.debug_copy_index("cent_f16", np.empty((nlist, dim), np.uint16))
            assert np.array_equal(case.cbits, fb.f16_image(case.cent)), "cent_f16 differs from the restated image of the centroids"
            case.cresid = case.idx.debug_copy_index("cent_f16_resid", np.empty(nlist, np.float32))
            ok = fb.residual_ok(case.cresid, fb.resid64(case.cent, case.cbits))
            assert ok.all(), f"cent_f16_resid off for lists {np.nonzero(~ok)[0][:10]}"
            case.rc_max, case.cnorm_max = fb.rc_max_of(case.cresid), fb.cnorm_max_of(case.cnorm2)
            case.qualifies = fb.gate(case.cresid, case.cnorm2)
            cache[k] = case
        return cache[k]
    yield get, stream
    for c in cache.values():
        c.close()


def _operands(case, nq, nprobe=NPROBE):
    return case.idx.stage_resources(nq, TOP_K, nprobe)["rank"]["operands"]


def _check_call(case, stream, nq, what, seed=0, sample=4096):
    """(a) query side, (b), (c) of the call that just ran on `stream`.  Returns the score rows."""
    idx, D, nlist, metric = case.idx, case.D, case.nlist, case.metric
    s = stream.cuda_stream
    A = idx.debug_copy_workspace(s, "scores", np.empty((nq, nlist), np.float32))
    rot = idx.debug_copy_workspace(s, "rot", np.empty((nq, D), np.float32))
    consts = idx.debug_copy_workspace(s, "consts", np.empty((nq, 12), np.float32))
    qbits = idx.debug_copy_workspace(s, "rot_f16", np.empty((nq, D), np.uint16))
    rq = idx.debug_copy_workspace(s, "rank_resid", np.empty(nq, np.float32))
    bad = np.nonzero((qbits != fb.f16_image(rot)).any(1))[0]
    assert bad.size == 0, f"{what}: rot_f16 differs from the restated image of rot for queries {bad[:10]}"
    ok = fb.residual_ok(rq, fb.resid64(rot, qbits))
    assert ok.all(), f"{what}: rank_resid off for queries {np.nonzero(~ok)[0][:10]}"
    worst, viol, skipped = fb.check_rows(A, rot, case.cent, metric, D, skip_rewritten=True, qbits=qbits, cbits=case.cbits)
    print(f"{what}: worst |A - s64| / budget = {worst:.4f}" + (f" ({skipped} rescored IP entries left out)" if skipped else ""))
    assert not viol, f"{what}: {len(viol)} score(s) outside the GEMM budget, first (q, list) {viol[0]}"
    n = nq * nlist
    flat = np.arange(n) if n <= 65536 else np.random.default_rng(seed).choice(n, sample, replace=False)
    qi, ci = flat // nlist, flat % nlist
    canon = rb.canonical(rot[qi], case.cent[ci], metric)
    eps = fb.select_eps(D, consts[qi, 6], case.cnorm2_max, rq[qi], case.cnorm_max, case.rc_max).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        over = ~(np.abs(A[qi, ci].astype(np.float64) - canon.astype(np.float64)) <= eps)
    if over.any() and metric == 1:
        over[over] = ~rb.rewritten(A, rot, case.cent, qi[over], ci[over])
    assert not over.any(), f"{what}: |A - canonical| > eps at (q, list) {list(zip(qi[over][:5].tolist(), ci[over][:5].tolist()))}"
    return A


def _oracle(case, q, res, what, nprobe=NPROBE):
    ids, sc, cnt = res
    hids, hsc, hcnt = _compare(case.built, case.idx, q, TOP_K, nprobe)
    assert np.array_equal(cnt, hcnt), f"{what}: device-call counts differ from the oracle's"
    bad = np.nonzero((ids != hids).any(axis=1))[0]
    assert bad.size == 0, f"{what}: device-call ids differ from the oracle's for queries {bad[:10]}"
    for i in range(q.shape[0]):
        np.testing.assert_allclose(sc[i, :cnt[i]], hsc[i, :cnt[i]], rtol=RTOL, atol=0)


def _reset(case):
    case.idx.set_option("rank_f16", -1)
    _set(case.idx, {})


def _run(env, dim, nlist, nq, tile, metric, oracle=False):
    get, stream = env
    case = get(dim, nlist, metric)
    what = f"f16 D {dim} nlist {nlist} nq {nq} tile {tile} metric {metric}"
    assert case.qualifies, what
    q = _queries("mix", nq, dim, 11 + nq + dim)
    _set(case.idx, {"rank_tile": tile, "rank_ksplit": 0, **_prep_opts(nq)})
    case.idx.set_option("rank_f16", 1)
    try:
        assert _rank_workgroups(case.idx, nq, NPROBE) == _tiles(nlist, nq, tile), what
        assert _operands(case, nq) == "f16", what
        f0 = case.idx.rank_fallbacks()
        res = _device_search(case, stream, q, NPROBE)
        _check_call(case, stream, nq, what)                                       # (a) (b) (c)
        assert case.idx.rank_fallbacks() == f0, f"{what}: the shortlist fell back on ordinary data"  # (d)
        if oracle:                                                                # (e)
            _oracle(case, q, res, what)
    finally:
        _reset(case)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("nlist", NLISTS)
@pytest.mark.parametrize("dim", DIMS)
def test_tiles(env, dim, nlist, nq, tile, metric):
    _run(env, dim, nlist, nq, tile, metric)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("tile", TILES)
def test_results_match_oracle(env, tile, metric):
    _run(env, 192, 1000, 129, tile, metric, oracle=True)


@pytest.mark.parametrize("metric", [0, 1])
def test_by_rule(env, metric):
    """Default options at the smallest big call: the route is taken, holds its budget and the oracle; rank_f16 = 0 runs
    split-bf16 and returns the same ids, scores and counts."""
    get, stream = env
    dim, nlist, nq = 256, 3072, 1024
    case = get(dim, nlist, metric)
    what = f"f16 by rule metric {metric}"
    q = _queries("mix", nq, dim, 23)
    _reset(case)
    try:
        assert case.qualifies
        assert _operands(case, nq) == "f16" and _rank_workgroups(case.idx, nq, NPROBE) == _tiles(nlist, nq, 128)
        f0 = case.idx.rank_fallbacks()
        res = _device_search(case, stream, q, NPROBE)
        _check_call(case, stream, nq, what)
        assert case.idx.rank_fallbacks() == f0
        _oracle(case, q, res, what)
        # smaller than big, or a forced tile: split-bf16
        assert _operands(case, 896) == "bf16x3"  # (168 tiles)
        case.idx.set_option("rank_tile", 128)
        assert _operands(case, nq) == "bf16x3"
        case.idx.set_option("rank_tile", 0)
        case.idx.set_option("rank_f16", 0)
        assert _operands(case, nq) == "bf16x3" and _rank_workgroups(case.idx, nq, NPROBE) == _tiles(nlist, nq, 128)
        res0 = _device_search(case, stream, q, NPROBE)
        trb._check_row(case, stream, nq, "bf16x3 beside f16 by rule", True)
        for x, y in zip(res, res0):
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), what
    finally:
        _reset(case)


def test_by_rule_needs_d256(env):
    get, _ = env
    case = get(192, 1000, 0)
    _reset(case)
    assert _operands(case, 4096) == "bf16x3"  # (256 tiles of 128 x 128: big, but D < 256)


@pytest.mark.parametrize("kind", ["mix_1e-4", "mix_1e5"])
def test_gate_keeps_split_bf16(env, kind):
    """Centroid halves that flush (x 1e-4) or are not finite (x 1e5): the index does not qualify, a forced route stays on
    split-bf16, results equal the oracle's."""
    get, stream = env
    case = get(192, 129, 0, kind)
    nq = 129
    assert not case.qualifies
    if kind == "mix_1e-4":
        assert (((case.cbits & 0x7FFF) == 0) & (case.cent != 0)).any()
    else:
        assert ((case.cbits & 0x7FFF) == 0x7C00).any() and not np.isfinite(case.cresid).all()
    q = _queries("mix_1e-4", nq, 192, 31) if kind == "mix_1e-4" else (_queries("mix", nq, 192, 31) * np.float32(1e5)).astype(np.float32)
    _set(case.idx, {"latency_path": 0})
    case.idx.set_option("rank_f16", 1)
    try:
        assert _operands(case, nq) == "bf16x3"
        res = _device_search(case, stream, q, NPROBE)
        trb._check_row(case, stream, nq, f"gate {kind}", True)
        _oracle(case, q, res, f"gate {kind}")
    finally:
        _reset(case)


def test_query_image_not_finite_falls_back(env):
    """Queries x 1e6 on an ordinary index: halves of the query image are inf, |q - f16(q)| and eps are not finite, every such
    query takes the canonical fallback; results equal the oracle's."""
    get, stream = env
    case = get(192, 1000, 0)
    nq = 129
    q = (_queries("mix", nq, 192, 37) * np.float32(1e6)).astype(np.float32)
    _set(case.idx, {"latency_path": 0})
    case.idx.set_option("rank_f16", 1)
    try:
        assert _operands(case, nq) == "f16"
        f0 = case.idx.rank_fallbacks()
        res = _device_search(case, stream, q, NPROBE)
        s = stream.cuda_stream
        rot = case.idx.debug_copy_workspace(s, "rot", np.empty((nq, 192), np.float32))
        qbits = case.idx.debug_copy_workspace(s, "rot_f16", np.empty((nq, 192), np.uint16))
        rq = case.idx.debug_copy_workspace(s, "rank_resid", np.empty(nq, np.float32))
        assert np.array_equal(qbits, fb.f16_image(rot))
        bad = ((qbits & 0x7C00) == 0x7C00).any(1)
        assert bad.any() and np.array_equal(~np.isfinite(rq), bad)
        assert case.idx.rank_fallbacks() - f0 >= int(bad.sum())
        _oracle(case, q, res, "queries x 1e6")
    finally:
        _reset(case)


@pytest.mark.parametrize("metric", [0, 1])
def test_far_queries(env, metric):
    """Queries 100 x farther out than the data: finite images, every score inside the budget and eps, the oracle's results."""
    get, stream = env
    case = get(192, 1000, metric)
    nq = 129
    q = _queries("far", nq, 192, 41)
    _set(case.idx, {"latency_path": 0})
    case.idx.set_option("rank_f16", 1)
    try:
        assert _operands(case, nq) == "f16"
        res = _device_search(case, stream, q, NPROBE)
        _check_call(case, stream, nq, f"far queries metric {metric}")
        _oracle(case, q, res, f"far queries metric {metric}")
    finally:
        _reset(case)
