"""The ranking GEMM's approximate scores A against the float64 bound of the rank_mfma.hpp header.

Every search ranks the IVF centroids with an approximate GEMM and rescores a shortlist exactly, so final results hide a
GEMM that is slightly wrong (exact rescoring repairs the order) or badly wrong (every query falls back to the canonical
ranking of all lists).  These tests read the score row itself after a full rbq_search_batch_device call and hold every
(query, list) entry to the GEMM's share of the header's budget (tests/rank_bound.py), on every GEMM route, at ragged tile
edges and over magnitudes from 1e-4 to 1e4; a sample is also held to the selector's own claim |A - canonical| <= eps.
The split-bf16 operands (workspace "rot_hi" / "rot_lo", index "cent_hi" / "cent_lo") must equal a numpy restatement of
bf16_split bit for bit, and the results must equal the oracle's.  Run with -s to see the worst error / budget per route."""
import numpy as np
import pytest

import rabitq_rs_amd as rq
import rank_bound as rb
from conftest import make_dataset
from test_gpu_parity import RTOL, _compare

pytestmark = pytest.mark.gpu

TOP_K = 10
DEFAULTS = {"rank_tile": 0, "rank_ksplit": 1, "f32_rank": 0, "wg_prep": 0, "latency_path": 1, "stage_mask": 15}
_WORST = {}  # route -> largest |A - s64| / budget seen


def _data(kind, n, dim, seed):
    x = make_dataset(n, dim, 16, seed)
    if kind == "mix":
        return x
    if kind == "mix_1e-4":
        return (x * np.float32(1e-4)).astype(np.float32)
    if kind == "mix_1e4":
        return (x * np.float32(1e4)).astype(np.float32)
    if kind == "int255":
        return np.random.default_rng(seed).integers(0, 256, (n, dim)).astype(np.float32)
    if kind == "coord_scales":  # per-coordinate scales 1e-3 .. 1e3
        return (x * np.logspace(-3, 3, dim, dtype=np.float32)[None, :]).astype(np.float32)
    if kind == "offset":  # |q|^2 + |c|^2 dwarfs every difference
        return (x + np.float32(1e3)).astype(np.float32)
    raise ValueError(kind)


def _queries(kind, nq, dim, seed):
    if kind == "far":  # 100x farther out than the data ("mix")
        return (make_dataset(nq, dim, 16, seed) * np.float32(100.0)).astype(np.float32)
    return _data(kind, nq, dim, seed)


class _Case:
    """One index (built once per module) and what the GEMM reads of it."""

    def __init__(self, dim, nlist, metric, rotator, kind):
        import torch
        seed = 1000 + dim * 7 + nlist * 13 + metric * 3 + rotator + len(kind)
        n = max(2000, 3 * nlist)
        data = _data(kind, n, dim, seed)
        rng = np.random.default_rng(seed + 1)
        cent = data[rng.choice(n, nlist, replace=False)].copy()
        x, c = torch.from_numpy(data).cuda(), torch.from_numpy(cent).cuda()
        assign = torch.cat([torch.cdist(x[i:i + 8192], c).argmin(dim=1) for i in range(0, n, 8192)])
        self.built = rq.builder.train_with_clusters(data, cent, assign.cpu().numpy().astype(np.uint32), 3, metric, rotator,
                                                    seed + 2, True)
        self.idx = rq.IvfRabitqIndex.from_built(self.built)
        self.dim, self.nlist, self.metric, self.kind = dim, nlist, metric, kind
        self.D = int(self.built.padded_dim)
        D = self.D
        self.cent = self.idx.debug_copy_index("centroids", np.empty((nlist, D), np.float32))
        self.cnorm2 = self.idx.debug_copy_index("cnorm2", np.empty(nlist, np.float32))
        ch = self.idx.debug_copy_index("cent_hi", np.empty((nlist, D), np.uint16))
        cl = self.idx.debug_copy_index("cent_lo", np.empty((nlist, D), np.uint16))
        # the operands of the split-bf16 GEMM are bf16_split of the centroids, bit for bit, and the split's residual is bounded
        wh, wl = rb.bf16_split(self.cent)
        assert np.array_equal(ch, wh) and np.array_equal(cl, wl), "cent_hi / cent_lo differ from bf16_split(centroids)"
        assert rb.split_residual_ok(self.cent, ch, cl).all()
        ref = np.stack([self.built.centroid(i) for i in range(nlist)])
        assert np.array_equal(self.cent.view(np.uint32), ref.view(np.uint32)), "device centroids differ from the built index"
        # cnorm2 feeds the L2 score: held to the same float64 bound as the GEMM's norm terms
        c64 = self.cent.astype(np.float64)
        n64 = (c64 * c64).sum(1)
        assert (np.abs(self.cnorm2 - n64) <= (D + 2) * rb.U * n64).all()
        self.cnorm2_max = rb.cnorm2_max_of(self.cnorm2)

    def close(self):
        self.idx.close()
        self.built.close()


@pytest.fixture(scope="module")
def env():
    import torch
    cache = {}
    stream = torch.cuda.Stream(torch.device("cuda", 0))

    def get(dim, nlist, metric=0, rotator=1, kind="mix"):
        k = (dim, nlist, metric, rotator, kind)
        if k not in cache:
            cache[k] = _Case(*k)
        return cache[k]
    yield get, stream
    print("\nranking GEMM: largest |A - s64| / budget per route")
    for route in sorted(_WORST):
        print(f"  {route:<40s} {_WORST[route]:.4f}")
    for c in cache.values():
        c.close()


def _set(idx, opts):
    for k, v in {**DEFAULTS, **opts}.items():
        idx.set_option(k, v)


def _device_search(case, stream, q, nprobe):
    """One rbq_search_batch_device call on `stream`; (ids, scores, counts) as numpy once it finished."""
    import torch
    dev = torch.device("cuda", 0)
    nq = q.shape[0]
    qd = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    d_ids = torch.zeros(nq, TOP_K, dtype=torch.int64, device=dev)
    d_sc = torch.zeros(nq, TOP_K, dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(nq, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    case.idx.search_batch_device(qd.data_ptr(), nq, case.dim, TOP_K, nprobe, d_ids.data_ptr(), d_sc.data_ptr(),
                                 d_cnt.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    return d_ids.cpu().numpy().view(np.uint64), d_sc.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32)


def _check_row(case, stream, nq, route, split, sample=4096, seed=0):
    """Read the score row of the call that just ran on `stream` and hold it to the bound.  Returns the row."""
    idx, D, nlist, metric = case.idx, case.D, case.nlist, case.metric
    A = idx.debug_copy_workspace(stream.cuda_stream, "scores", np.empty((nq, nlist), np.float32))
    rot = idx.debug_copy_workspace(stream.cuda_stream, "rot", np.empty((nq, D), np.float32))
    consts = idx.debug_copy_workspace(stream.cuda_stream, "consts", np.empty((nq, 12), np.float32))
    if split:  # the query half of the split-bf16 operands
        rh = idx.debug_copy_workspace(stream.cuda_stream, "rot_hi", np.empty((nq, D), np.uint16))
        rl = idx.debug_copy_workspace(stream.cuda_stream, "rot_lo", np.empty((nq, D), np.uint16))
        wh, wl = rb.bf16_split(rot)
        bad = np.nonzero((rh != wh).any(1) | (rl != wl).any(1))[0]
        assert bad.size == 0, f"{route}: rot_hi / rot_lo differ from bf16_split(rot) for queries {bad[:10]}"
        assert rb.split_residual_ok(rot, rh, rl).all()
    worst, viol, skipped = rb.check_rows(A, rot, case.cent, metric, D, skip_rewritten=True)
    _WORST[route] = max(_WORST.get(route, 0.0), worst)
    print(f"{route}: D={D} nlist={nlist} nq={nq} worst |A - s64| / budget = {worst:.4f}"
          + (f" ({skipped} rescored IP entries left out)" if skipped else ""))
    if viol:
        qi, ci = viol[0]
        s64, norms = rb.exact_scores(rot[qi:qi + 1], case.cent[ci:ci + 1], metric)
        pytest.fail(f"{route}: {len(viol)} score(s) outside the GEMM budget, first (q {qi}, list {ci}): A={A[qi, ci]!r} "
                    f"s64={s64[0, 0]!r} budget={rb.gemm_budget(D, norms)[0, 0]!r}")
    # the selector's own claim on a sample: |A - canonical| <= eps
    n = nq * nlist
    flat = np.arange(n) if n <= 65536 else np.random.default_rng(seed).choice(n, sample, replace=False)
    qi, ci = flat // nlist, flat % nlist
    canon = rb.canonical(rot[qi], case.cent[ci], metric)
    eps = rb.select_eps(D, consts[qi, 6], case.cnorm2_max).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        over = ~(np.abs(A[qi, ci].astype(np.float64) - canon.astype(np.float64)) <= eps)
    if over.any() and metric == 1:
        over[over] = ~rb.rewritten(A, rot, case.cent, qi[over], ci[over])
    assert not over.any(), (f"{route}: |A - canonical| > eps at (q, list) "
                            f"{list(zip(qi[over][:5].tolist(), ci[over][:5].tolist()))}")
    return A


def _rank_workgroups(idx, nq, nprobe):
    return idx.stage_resources(nq, TOP_K, nprobe)["rank"]["workgroups"]


def _tiles(nlist, nq, tile):
    bm, bn = (128, 256) if tile == 256 else (tile, tile)
    return -(-nlist // bn) * -(-nq // bm)


def _run(env, *, dim, nlist, nq, route, opts=(), metric=0, rotator=1, kind="mix", qkind=None, nprobe=16,
         tile=None, ksplit=1, no_fallback=True, compare=True):
    get, stream = env
    case = get(dim, nlist, metric, rotator, kind)
    q = _queries(qkind or kind, nq, dim, 7 + nq + dim)
    nprobe = min(nprobe, nlist)
    opts = dict(opts)
    _set(case.idx, opts)
    try:
        split = case.D % 64 == 0 and not opts.get("f32_rank", 0)
        if tile is not None:  # the route the test means to reach is the one the call launches
            assert _rank_workgroups(case.idx, nq, nprobe) == _tiles(nlist, nq, tile) * ksplit, route
        f0 = case.idx.rank_fallbacks()
        ids, sc, cnt = _device_search(case, stream, q, nprobe)
        _check_row(case, stream, nq, route, split)
        if opts.get("stage_mask", 15) != 15:
            return case
        if no_fallback:
            assert case.idx.rank_fallbacks() == f0, f"{route}: the shortlist fell back on ordinary data"
        if compare:
            # the host path against the oracle; the device call must then give the oracle's ids and counts as well
            hids, hsc, hcnt = _compare(case.built, case.idx, q, TOP_K, nprobe)
            assert np.array_equal(cnt, hcnt), f"{route}: device-call counts differ from the oracle's"
            bad = np.nonzero((ids != hids).any(axis=1))[0]
            assert bad.size == 0, f"{route}: device-call ids differ from the oracle's for queries {bad[:10]}"
            for i in range(nq):
                np.testing.assert_allclose(sc[i, :cnt[i]], hsc[i, :cnt[i]], rtol=RTOL, atol=0)
    finally:
        _set(case.idx, {})
    return case


# ---- the split-bf16 GEMM's tiles --------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("tile", [64, 128, 256])
def test_bf16_tiles(env, tile, metric):
    """rank_tile 64 / 128 / 256 at a ragged shape (1000 lists, 1025 queries: the last row and column tiles are partial)."""
    _run(env, dim=128, nlist=1000, nq=1025, metric=metric, opts={"rank_tile": tile}, tile=tile,
         route=f"bf16 tile {tile} metric {metric}")


@pytest.mark.parametrize("nlist,nq,tile", [
    (1, 5, None), (2, 31, 64), (63, 33, 64), (65, 65, 128), (129, 255, 256), (257, 256, 64), (1000, 257, 128),
    (63, 513, 256), (65, 1024, 64), (257, 129, 128),
])
def test_ragged_tile_edges(env, nlist, nq, tile):
    """Partial tiles in both directions; rank_tile forced round the three tiles (None: by size)."""
    opts = {"rank_tile": tile} if tile else {}
    t = tile or 64  # (by size, these shapes are small: 64 x 64)
    _run(env, dim=128, nlist=nlist, nq=nq, opts=opts, tile=t, route=f"bf16 tile {t} ragged")


def test_rank_tile_by_size_picks_128(env):
    """rank_tile 0 with enough 128 x 128 tiles to fill the chip (nlist > 4096: the selector keeps the row in LDS)."""
    _run(env, dim=64, nlist=5000, nq=1024, tile=128, route="bf16 tile 128 (by size), nlist 5000")


def test_wide_tile_global_row_mode(env):
    """nlist > 16384: the selector re-reads the row from global memory; 128 x 256 tiles."""
    _run(env, dim=64, nlist=17000, nq=1024, opts={"rank_tile": 256}, tile=256, route="bf16 tile 256, nlist 17000")


# ---- split-K ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [64, 128, 960, 2048])
@pytest.mark.parametrize("ks", [2, 4])
def test_split_k(env, dim, ks):
    """rank_ksplit 2 / 4 behind the workgroup-per-query preparation: D 64 leaves parts with no slab (4 parts of 2 slabs),
    D 960 splits 30 slabs 8/8/8/6."""
    _run(env, dim=dim, nlist=257, nq=65, opts={"rank_ksplit": ks}, tile=64, ksplit=ks, route=f"split-K {ks}")


@pytest.mark.parametrize("dim,nq", [(960, 31), (2048, 200)])
def test_split_k_by_size(env, dim, nq):
    """The default choice (4 parts for a handful of tiles) at D 960 and 2048, L2 and IP."""
    for metric in (0, 1):
        _run(env, dim=dim, nlist=257, nq=nq, metric=metric, tile=64, ksplit=4, route=f"split-K 4 (by size) metric {metric}")


def test_split_k_repeated_calls_clear_the_row(env):
    """Two split-K calls on one stream, the second with other queries: its row must be its own (a row not cleared
    before the atomic adds would hold the sum of both)."""
    get, stream = env
    case = get(960, 257)
    _set(case.idx, {"rank_ksplit": 4})
    try:
        for seed in (101, 202):
            q = _queries("mix", 65, 960, seed)
            _device_search(case, stream, q, 16)
            _check_row(case, stream, 65, "split-K 4, repeated calls", True)
        oids = _compare(case.built, case.idx, q, TOP_K, 16)[0]
        assert np.array_equal(_device_search(case, stream, q, 16)[0], oids)
    finally:
        _set(case.idx, {})


@pytest.mark.parametrize("ks", [8, 16])
def test_forced_split_is_clamped_to_four(env, ks):
    """rank_ksplit n > 4 launches 4 parts, the most eps is derived for; results equal the oracle."""
    get, _ = env
    case = get(960, 257)
    _set(case.idx, {"rank_ksplit": 4})
    four = _rank_workgroups(case.idx, 65, 16)
    _set(case.idx, {})
    assert four == _tiles(257, 65, 64) * 4
    _run(env, dim=960, nlist=257, nq=65, opts={"rank_ksplit": ks}, tile=64, ksplit=4, route=f"split-K {ks} (clamped to 4)")


def test_split_k_workgroups_are_counted(env):
    """stage_resources counts the grid.z parts of a split-K GEMM; the rest of what it reports of that kernel (the same
    instantiation with and without parts) does not change."""
    get, _ = env
    case = get(960, 257)
    try:
        res = {}
        for ks in (0, 2, 4):
            _set(case.idx, {"rank_ksplit": ks})
            res[ks] = case.idx.stage_resources(65, TOP_K, 16)
    finally:
        _set(case.idx, {})
    wg = {ks: r["rank"]["workgroups"] for ks, r in res.items()}
    assert wg[0] == _tiles(257, 65, 64)
    assert wg[2] == 2 * wg[0] and wg[4] == 4 * wg[0], wg
    for ks in (2, 4):
        for stage in ("prep", "rank", "select", "scan"):
            a, b = dict(res[0][stage]), dict(res[ks][stage])
            if stage == "rank":
                a.pop("workgroups"), b.pop("workgroups")
            assert a == b, (ks, stage, a, b)
    for stage, r in res[4].items():
        assert r["threads"] > 0 and r["vgprs"] > 0 and r["workgroups"] > 0, (stage, r)


# ---- the f32 MFMA GEMM --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", [0, 1])
def test_f32_rank(env, metric):
    """f32_rank=1: k_rank_mfma with 64 x 64 tiles, and with 128 x 128 ones at a shape that fills the chip."""
    _run(env, dim=128, nlist=1000, nq=1025, metric=metric, opts={"f32_rank": 1}, tile=64, route=f"f32 tile 64 metric {metric}")
    _run(env, dim=64, nlist=5000, nq=1024, metric=metric, opts={"f32_rank": 1}, tile=128,
         route=f"f32 tile 128 metric {metric}")


@pytest.mark.parametrize("dim,nlist,metric", [(48, 65, 0), (80, 129, 1), (1008, 257, 0)])
def test_matrix_rotator_f32_route(env, dim, nlist, metric):
    """The Matrix rotator at D % 64 != 0 ranks with the f32 GEMM (its K loop ends inside a slab)."""
    _run(env, dim=dim, nlist=nlist, nq=129, metric=metric, rotator=0, tile=64, route=f"f32 matrix rotator metric {metric}")


# ---- the three producers of the query operands ------------------------------------------------------------------

@pytest.mark.parametrize("opts,nq,route", [
    ({"wg_prep": 1}, 129, "prep k_prep (wg_prep=1)"),
    ({"latency_path": 0}, 129, "prep k_prep_wave (latency_path=0)"),
    ({}, 129, "prep k_lat_front"),
    ({}, 513, "prep k_prep_wave (nq > 512)"),
])
def test_query_preparation_routes(env, opts, nq, route):
    for metric in (0, 1):
        _run(env, dim=128, nlist=257, nq=nq, metric=metric, opts=opts, tile=64, route=f"{route} metric {metric}")


# ---- magnitudes ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,qkind,metric", [
    ("mix_1e-4", None, 0), ("mix_1e4", None, 0), ("mix_1e4", None, 1), ("int255", None, 0),
    ("coord_scales", None, 0), ("coord_scales", None, 1), ("mix", "far", 0), ("mix", "far", 1),
])
def test_magnitudes(env, kind, qkind, metric):
    """The bound scales with |q|^2 + |c|^2: tiny, huge, integer, anisotropic data and far-out queries, on the
    split-bf16 GEMM (with split-K) and on the f32 one."""
    tag = f"{kind}{'/' + qkind if qkind else ''} metric {metric}"
    _run(env, dim=128, nlist=129, nq=65, metric=metric, kind=kind, qkind=qkind, opts={"rank_ksplit": 4}, tile=64, ksplit=4,
         route=f"split-K 4, {tag}")
    _run(env, dim=128, nlist=129, nq=129, metric=metric, kind=kind, qkind=qkind, opts={"f32_rank": 1}, tile=64,
         route=f"f32, {tag}")


@pytest.mark.parametrize("metric", [0, 1])
def test_common_offset(env, metric):
    """Data and queries offset by 1e3: |q|^2 + |c|^2 dwarfs the differences, the shortlist may overflow and fall back
    (which rewrites the row with canonical scores).  The bound and exact results hold; the GEMM rows themselves are
    read with the selection and scan stages switched off."""
    for opts, route in (({}, "bf16"), ({"f32_rank": 1}, "f32")):
        _run(env, dim=128, nlist=129, nq=129, metric=metric, kind="offset", opts=opts, no_fallback=False,
             route=f"{route}, offset 1e3 metric {metric}")
        _run(env, dim=128, nlist=129, nq=129, metric=metric, kind="offset", opts={**opts, "stage_mask": 3},
             route=f"{route}, offset 1e3 metric {metric} (row before selection)")
