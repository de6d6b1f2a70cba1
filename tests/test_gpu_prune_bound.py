"""The scan's pruning bounds against the oracle's own per-vector values (tests/prune_bound.py).

The scan skips nearly every probed block on the block bound lbmin of its stream entry, and the lazy selection drops whole
lists; all of it rests on GPU-only quantities the oracle never computes.  These tests read them back and hold each to its
claim over EVERY vector it covers:
  * bsum / lsum / bsumx (k_block_summary, k_list_summaries) against a restatement from the reference-layout codes;
  * every stream entry of k_select_mfma (eager and lazy, every preparation kernel, every numeric variant) and of k_select
    (exact_rank, nprobe beyond the LDS key window): lbmin <= lb_v of every real vector, lb_v from oracle.list_vectors with
    the reference's own g_add / g_err, and the entries are exactly the probed lists' blocks in probe order;
  * QueryConsts: accu and the ex-code dot of every probed vector inside [amin, amax] / [exlo, exhi];
  * single-vector blocks whose code reaches amin (amax): lbmin must equal lb_v bit for bit, under each variant;
  * the lazy selection's head bounds (option ub_tap): U >= max(dist_v, lb_v) for every real vector of every head block, and
    T_ub is the rule's value over the tapped bounds; each rounding-slack term of block_ub is required on some index.
Run with -s to see the worst lb_v - lbmin gap per case."""
import numpy as np
import pytest

import oracle
import prune_bound as pb
import rabitq_rs_amd as rq
from conftest import make_dataset

pytestmark = pytest.mark.gpu

F32 = np.float32
TOP_K = 10
MASK = {"native_avx512": 0, "native_avx2": 1, "portable": 6}  # the oracle variant each GPU variant reproduces
AUDIT_ROW = 1024  # kAuditCap + 1 words per query of the "audit_dead" workspace buffer
_GAPS = {}


def _clustered(sizes, dim, seed, scales=None):
    """Data with the given list sizes (a crafted clustering: list c holds the vectors assigned to it), scaled per list."""
    rng = np.random.default_rng(seed)
    nl = len(sizes)
    scales = scales if scales is not None else np.ones(nl)
    cent = (rng.standard_normal((nl, dim)) * 3).astype(F32)
    data, assign = [], []
    for c, n in enumerate(sizes):
        x = cent[c] + rng.standard_normal((n, dim)).astype(F32)
        data.append((x * F32(scales[c])).astype(F32))
        cent[c] = cent[c] * F32(scales[c])
        assign += [c] * n
    return np.concatenate(data).astype(F32), cent, np.array(assign, np.uint32)


def _summaries(idx, nblocks, nlist):
    return (idx.debug_copy_index("bsum", np.empty((nblocks, 8), F32)), idx.debug_copy_index("lsum", np.empty((nlist, 8), F32)),
            idx.debug_copy_index("bsumx", np.empty((nblocks, 8), F32)))


def _check_index_summaries(idx, host, what):
    lists = pb.lists_of(host)
    D, ex = int(host.padded_dim), int(host.header.ex_bits)
    r = pb.restate(lists, D, ex)
    nl = len(lists)
    gb0 = idx.debug_copy_index("list_gb0", np.empty(nl, np.uint32))
    ln = idx.debug_copy_index("list_n", np.empty(nl, np.uint32))
    assert np.array_equal(ln, [len(a["ids"]) for a in lists]), what
    assert np.array_equal(gb0, r.gb0), f"{what}: device list_gb0 differs from the lists' block prefix"
    viol, worst = pb.check_summaries(r, *_summaries(idx, r.bsum.shape[0], nl))
    assert not viol, f"{what}: {len(viol)} summary violation(s): {viol[:5]}"
    return r, worst


SIZES = [0, 1, 31, 32, 33, 64, 65]


@pytest.mark.parametrize("bits", [1, 3, 7])
@pytest.mark.parametrize("dim", [1, 15, 63, 65, 128, 960, 2048])
def test_summaries_fht_kac(bits, dim):
    data, cent, assign = _clustered(SIZES, dim, dim * 10 + bits, scales=np.logspace(-4, 4, len(SIZES)))
    built = rq.builder.train_with_clusters(data, cent, assign, bits, 0, 1, dim + bits, True)
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        _, worst = _check_index_summaries(idx, built, f"fht-kac dim {dim} bits {bits}")
        assert worst <= 3
    finally:
        idx.close()
        built.close()


@pytest.mark.parametrize("rotator,dim,bits", [(0, 16, 7), (0, 1008, 3), (2, 64, 7), (2, 64, 1)])
def test_summaries_matrix_and_none(rotator, dim, bits):
    data, cent, assign = _clustered(SIZES, dim, dim + rotator, scales=np.logspace(-4, 4, len(SIZES)))
    built = rq.builder.train_with_clusters(data, cent, assign, bits, 1, rotator, 5, True)
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        _check_index_summaries(idx, built, f"rotator {rotator} dim {dim}")
    finally:
        idx.close()
        built.close()


def test_summaries_of_rbq1_with_non_finite_factors():
    """RBQ1 bytes (tests/rbq1_writer.py) with an inf f_add and a NaN f_rescale: their blocks and lists become unusable,
    the others keep exact ranges."""
    data, cent, assign = _clustered([40, 70, 33, 5], 128, 17)
    built = rq.builder.train_with_clusters(data, cent, assign, 7, 0, 1, 3, True)
    host = pb.host_index_of(built)
    built.close()
    D = 128
    s = pb.record_stride(D)
    c0 = host.clusters[0]["batch_data"]
    c0[s + D * 4 + 4 * 2:s + D * 4 + 4 * 3] = np.array([np.inf], F32).view(np.uint8)            # f_add of vector 34 (block 1)
    c2 = host.clusters[2]["batch_data"]
    c2[D * 4 + 4 * (32 + 7):D * 4 + 4 * (32 + 8)] = np.array([np.nan], F32).view(np.uint8)      # f_rescale of vector 7 (block 0)
    idx = rq.IvfRabitqIndex.load_from_bytes(host.rbq1())
    try:
        r, _ = _check_index_summaries(idx, host, "rbq1 non-finite")
        assert list(r.bsum_ok) == [True, False, True, True, True, False, True, True] and list(r.lsum_ok) == [False, True, False, True]
    finally:
        idx.close()


# ---- the block stream ------------------------------------------------------------------------------------------------

class _Env:
    def __init__(self):
        import torch
        self.torch = torch
        self.stream = torch.cuda.Stream(torch.device("cuda", 0))
        self.cache = {}

    def index(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]


@pytest.fixture(scope="module")
def env():
    e = _Env()
    yield e
    print("\nblock bound: worst lb_v - lbmin (absolute, relative), finite / sharp entries per case")
    for k in sorted(_GAPS):
        print(f"  {k:<44s} {_GAPS[k]}")
    for built, idx, _ in e.cache.values():
        idx.close()
        built.close()


def _make(dim, nlist, n, bits, metric, scale=1.0, seed=0):
    def make():
        data = (make_dataset(n, dim, max(nlist // 4, 1), seed + dim + bits) * F32(scale)).astype(F32)
        built = rq.builder.train(data, nlist, bits, metric, 1, seed + 7, True, kmeans_iters=4)
        return built, rq.IvfRabitqIndex.from_built(built), data
    return make


def _device_search(env, idx, q, nprobe, top_k=TOP_K):
    torch = env.torch
    dev = torch.device("cuda", 0)
    nq, dim = q.shape
    qd = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    d_ids = torch.zeros(nq, top_k, dtype=torch.int64, device=dev)
    d_sc = torch.zeros(nq, top_k, dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(nq, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    idx.search_batch_device(qd.data_ptr(), nq, dim, top_k, nprobe, d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr(),
                            stream=env.stream.cuda_stream)
    env.stream.synchronize()
    return d_ids.cpu().numpy().view(np.uint64), d_sc.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32)


def _wl_stride(built, nprobe):
    nb = np.sort((built.list_sizes() + 31) // 32)[::-1]
    return max(int(nb[:nprobe].sum()), 1)


def _taps(env, idx, built, nq, nprobe, audit):
    st = env.stream.cuda_stream
    ws = _wl_stride(built, nprobe)
    t = {"consts": idx.debug_copy_workspace(st, "consts", np.empty((nq, 12), F32)),
         "probe": idx.debug_copy_workspace(st, "probe", np.empty((nq, nprobe, 4), np.uint32)),
         "nstream": idx.debug_copy_workspace(st, "nstream", np.empty(nq, np.uint32)),
         "wl": idx.debug_copy_workspace(st, "wl", np.empty((nq, ws, 4), np.uint32)),
         "dead": idx.debug_copy_workspace(st, "dead_skipped", np.empty((4, nq), np.uint32))}
    if audit:
        t["audit"] = idx.debug_copy_workspace(st, "audit_dead", np.empty((nq, AUDIT_ROW), np.uint32))
    return t


def _check_stream_case(env, key, make, nq, nprobe, opts, variant="native_avx512", select_mfma=True, label=None):
    built, idx, data = env.index(key, make)
    label = label or f"{key} nq={nq} {opts} {variant}"
    rng = np.random.default_rng(nq + nprobe)
    q = (data[rng.choice(len(data), nq, replace=nq > len(data))] +
         F32(0.1) * np.abs(data).mean() * rng.standard_normal((nq, data.shape[1])).astype(F32)).astype(F32)
    base = {"lazy_select": 1, "lazy_audit": 0, "exact_rank": 0, "latency_path": 1, "wg_prep": 0}
    for k, v in {**base, **opts}.items():
        idx.set_option(k, v)
    idx.set_numeric_variant(variant)
    lists = pb.lists_of(built)
    rest = pb.restate(lists, int(built.padded_dim), int(built.header.ex_bits))
    try:
        ids, sc, cnt = _device_search(env, idx, q, nprobe)
        t = _taps(env, idx, built, nq, nprobe, opts.get("lazy_audit", 0))
    finally:
        for k, v in base.items():
            idx.set_option(k, v)
        idx.set_numeric_variant("native_avx512")
    with oracle.variant(MASK[variant]):
        rc, oids, osc, ocnt, _ = oracle.search_batch(built, q, TOP_K, nprobe)
        assert rc == 0
        assert np.array_equal(cnt, ocnt), f"{label}: counts differ from the oracle's"
        assert all(np.array_equal(ids[i, :cnt[i]], oids[i, :cnt[i]]) for i in range(nq)), f"{label}: ids differ from the oracle's"
        eager = not select_mfma or not opts.get("lazy_select", 1)
        total, bad, skipped_bound = pb.StreamStats(), [], 0
        for i in range(nq):
            rqv = oracle.rotate(built, q[i])
            cids = oracle.select_probes(built, rqv, nprobe)
            plan = pb.probe_plan(built, lists, rest, rqv, cids, oracle)
            c = t["consts"][i]
            viol = pb.check_consts(c, rqv, np.concatenate([p["accu"] for p in plan]), np.concatenate([p["exdot"] for p in plan]),
                                   oracle.query_lut(rqv)[0])
            assert not viol, f"{label} query {i}: {viol}"
            if c[pb.QC["amax"]] > 65535.0:  # the scan switches the block bound off (accu may wrap): results only
                skipped_bound += 1
                continue
            np_ = int(t["dead"][1, i]) if select_mfma else nprobe
            scanned = t["probe"][i, :np_, 3].tolist()
            dropped = None
            if "audit" in t:
                a = t["audit"][i]
                assert a[0] < AUDIT_ROW, f"{label}: audit overflow"
                dropped = a[1:1 + a[0]].tolist()
            viol, st = pb.check_stream(t["wl"][i, :int(t["nstream"][i])], scanned, plan, eager=eager, dropped=dropped)
            if viol:
                bad.append((i, viol[:3]))
            total.add(st)
        assert not bad, f"{label}: {len(bad)} queries with stream violations, first {bad[:2]}"
    _GAPS[label] = (f"{total.worst_gap:.3g} ({total.worst_rel:.2g} rel)", f"{total.finite}/{total.entries} finite, "
                    f"{total.sharp} sharp", f"{skipped_bound} queries with amax > 65535")
    return total


IDX_A = ("A", 128, 64, 6000, 7, 0)   # (key, dim, nlist, n, bits, metric)
IDX_B = ("B", 960, 32, 2500, 3, 1)


def _mk(spec, scale=1.0):
    key, dim, nlist, n, bits, metric = spec
    return (key + f"@{scale:g}", dim, nlist, n, bits, metric), _make(dim, nlist, n, bits, metric, scale)


@pytest.mark.parametrize("nq,opts", [
    (1, {}), (4, {}), (5, {}), (200, {}), (600, {}), (5, {"latency_path": 0}), (5, {"wg_prep": 1}),
    (5, {"lazy_select": 0}), (200, {"lazy_select": 0}), (200, {"lazy_audit": 1}),
])
def test_stream_bound_select_mfma(env, nq, opts):
    key, make = _mk(IDX_A)
    _check_stream_case(env, key, make, nq, 16, opts)


@pytest.mark.parametrize("spec,scale", [(IDX_B, 1.0), (IDX_A, 1e-4), (IDX_A, 1e4), (IDX_B, 1e4)])
def test_stream_bound_shapes_and_scales(env, spec, scale):
    key, make = _mk(spec, scale)
    _check_stream_case(env, key, make, 64, 12, {"lazy_audit": 1})
    _check_stream_case(env, key, make, 64, 12, {"lazy_select": 0})


@pytest.mark.parametrize("variant", ["native_avx2", "portable"])
@pytest.mark.parametrize("lazy", [0, 1])
def test_stream_bound_numeric_variants(env, variant, lazy):
    key, make = _mk(IDX_A)
    _check_stream_case(env, key, make, 32, 16, {"lazy_select": lazy}, variant=variant)
    _check_stream_case(env, key, make, 32, 16, {"exact_rank": 1}, variant=variant, select_mfma=False)


@pytest.mark.parametrize("nq", [3, 300])
def test_stream_bound_k_select_exact_rank(env, nq):
    key, make = _mk(IDX_A)
    _check_stream_case(env, key, make, nq, 16, {"exact_rank": 1}, select_mfma=False)


def test_stream_bound_k_select_global_key_window(env):
    """nprobe > 8192: k_select with the key window in global memory, over 9000 tiny lists."""
    def make():
        rng = np.random.default_rng(4)
        nl, dim = 9000, 16
        cent = rng.standard_normal((nl, dim)).astype(F32)
        assign = np.concatenate([np.arange(nl), rng.integers(0, nl, 3000)]).astype(np.uint32)
        data = (cent[assign] + F32(0.05) * rng.standard_normal((len(assign), dim)).astype(F32)).astype(F32)
        built = rq.builder.train_with_clusters(data, cent, assign, 3, 0, 1, 11, True)
        return built, rq.IvfRabitqIndex.from_built(built), data
    _check_stream_case(env, "tiny9000", make, 2, 8500, {}, select_mfma=False)


# ---- the case that is sharp to the ulp -------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["native_avx512", "native_avx2", "portable"])
@pytest.mark.parametrize("metric", [0, 1])
def test_block_bound_is_exact_on_extreme_single_vector_blocks(env, variant, metric):
    """Single-vector lists whose sign code takes the argmin (f_rescale > 0) or argmax (f_rescale < 0) nibble of q0's LUT in
    every codebook: accu is then amin / amax, and block_lbmin evaluates the reference's own operation sequence on that
    vector's operands — lbmin must equal lb_v bit for bit (a fused / unfused mismatch or a reordered sum shows here)."""
    dim, n = 256, 48
    rng = np.random.default_rng(metric)
    data = (rng.standard_normal((n, dim)) * 2).astype(F32)
    cent = (data + F32(0.3) * rng.standard_normal((n, dim)).astype(F32)).astype(F32)
    built = rq.builder.train_with_clusters(data, cent, np.arange(n, dtype=np.uint32), 7, metric, 1, 21, True)
    host = pb.host_index_of(built)
    q0 = (data[0] * F32(0.5) + rng.standard_normal(dim).astype(F32)).astype(F32)
    rqv = oracle.rotate(built, q0)
    built.close()
    lut, _, _ = oracle.query_lut(rqv)
    amin, amax = pb.lut_range(lut)
    D = int(host.padded_dim)
    for c, cl in enumerate(host.clusters):
        fr = pb.block_factors(cl["batch_data"], D, 0)[1][0]
        codes = pb.pack_sign_bits(pb.extreme_bits(lut, fr > 0)[None, :], D)
        cl["batch_data"][:D * 4] = codes[:D * 4]
    idx = rq.IvfRabitqIndex.load_from_bytes(host.rbq1())
    try:
        idx.set_option("lazy_select", 0)
        idx.set_numeric_variant(variant)
        _device_search(env, idx, q0[None, :], n)
        t = _taps(env, idx, host, 1, n, False)
    finally:
        idx.close()
    with oracle.variant(MASK[variant]):
        lists = pb.lists_of(host)
        cids = oracle.select_probes(host, rqv, n)
        plan = pb.probe_plan(host, lists, pb.restate(lists, D, 6), rqv, cids, oracle)
    for p in plan:
        fr = pb.block_factors(host.clusters[p["cid"]]["batch_data"], D, 0)[1][0]
        assert int(p["accu"][0]) == (amin if fr > 0 else amax)
    items = t["wl"][0, :int(t["nstream"][0])]
    viol, st = pb.check_stream(items, t["probe"][0, :, 3].tolist(), plan)
    assert not viol, viol
    _, _, _, lbmin = pb.stream_items(items)
    lbv = np.array([p["lb"][0] for p in plan], F32)
    fin = np.isfinite(lbv)
    assert fin.sum() >= n - 2
    diff = np.nonzero(lbmin[fin].view(np.uint32) != lbv[fin].view(np.uint32))[0]
    assert diff.size == 0, f"{variant}: lbmin != lb_v at blocks {diff[:8]}: {lbmin[fin][diff[:3]]} vs {lbv[fin][diff[:3]]}"
    _GAPS[f"sharp metric {metric} {variant}"] = f"{int(fin.sum())} blocks, lbmin == lb_v bit for bit"


# ---- the lazy selection's head bounds (option ub_tap) ------------------------------------------------------------------

HEAD_ROW = 2 + 8 + 3 * 256  # kHeadUbRow
SLACK_TERMS = ("|q - c| <= g_err (1 + 1e-4)", "E_ip", "est rounding", "lb rounding", "ex-dot summation", "distance rounding")
_HEAD = {}


def _head_index(metric, bits, dim, scale):
    n, nlist = 3000, 24
    data = (make_dataset(n, dim, 6, 500 + dim + bits + metric) * F32(scale)).astype(F32)
    return data, rq.builder.train(data, nlist, bits, metric, 1, 31 + bits, True, kmeans_iters=4)


def _head_check(env, idx, host, data, label, nq=16, nprobe=8, seed=0, expect_clean=True):
    """One device search with ub_tap and head_exact 0; every query's head bounds against the oracle.  Returns (violations,
    stats)."""
    rng = np.random.default_rng(seed)
    q = (data[rng.choice(len(data), nq, replace=False)] +
         F32(0.05) * np.abs(data).mean() * rng.standard_normal((nq, data.shape[1])).astype(F32)).astype(F32)
    idx.set_option("head_exact", 0)
    idx.set_option("ub_tap", 1)
    try:
        _device_search(env, idx, q, nprobe)
        st = env.stream.cuda_stream
        row = idx.debug_copy_workspace(st, "head_ub", np.empty((nq, HEAD_ROW), np.uint32))
        dead = idx.debug_copy_workspace(st, "dead_skipped", np.empty((4, nq), np.uint32))
    finally:
        idx.set_option("ub_tap", 0)
        idx.set_option("head_exact", 1)
    lists = pb.lists_of(host)
    nbs = [(len(a["ids"]) + 31) // 32 for a in lists]
    owner = np.repeat(np.arange(len(lists)), nbs)
    gb0 = np.concatenate([[0], np.cumsum(nbs)[:-1]]).astype(np.int64)
    viol, ratios, nfin, ncands, queries = [], [], 0, 0, 0
    for i in range(nq):
        ncand, h = int(row[i, 0]), int(row[i, 1])
        if ncand == 0:
            continue
        queries += 1
        cands = [(int(row[i, 10 + 3 * j]), row[i, 11 + 3 * j:12 + 3 * j].view(F32)[0], int(row[i, 12 + 3 * j])) for j in range(ncand)]
        rqv = oracle.rotate(host, q[i])
        heads = list(dict.fromkeys(int(owner[c[0]]) for c in cands))
        assert len(heads) <= h <= 4, f"{label}: the candidates cover {len(heads)} lists, h = {h}"
        blocks = {}
        for r, cid in enumerate(heads):
            g_add, g_err = oracle.probe_geometry(host, rqv, cid)
            tg = row[i, 2 + 2 * r:4 + 2 * r].view(F32)
            if len(heads) == h and not (tg[0] >= g_add and tg[1] >= g_err):  # head_info takes both at the upper ends of their intervals
                viol.append(f"query {i} head list {cid}: g_add / g_err used ({tg[0]!r}, {tg[1]!r}) below the exact ({g_add!r}, {g_err!r})")
            v = oracle.list_vectors(host, rqv, cid, g_add, g_err)
            for b in range(nbs[cid]):
                blocks[int(gb0[cid]) + b] = (v["dist"][32 * b:32 * b + 32], v["lb"][32 * b:32 * b + 32])
        vq, stq = pb.check_head_ub(cands, blocks, dead[2, i:i + 1].view(F32)[0], TOP_K)
        viol += [f"query {i}: {x}" for x in vq]
        nfin += stq["finite"]
        ncands += stq["cands"]
        if np.isfinite(stq["median_ratio"]):
            ratios.append(stq["median_ratio"])
    return viol, {"queries": queries, "finite": nfin, "cands": ncands, "median_ratio": float(np.median(ratios)) if ratios else np.nan}


@pytest.mark.parametrize("scale", [1e-4, 1.0, 1e4])
@pytest.mark.parametrize("dim", [128, 960])
@pytest.mark.parametrize("bits", [1, 3, 7])
@pytest.mark.parametrize("metric", [0, 1])
def test_head_bounds_cover_every_vector(env, metric, bits, dim, scale):
    data, built = _head_index(metric, bits, dim, scale)
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        viol, st = _head_check(env, idx, built, data, f"metric {metric} bits {bits} D {dim} x{scale:g}")
    finally:
        idx.close()
        built.close()
    assert not viol, f"{len(viol)} head-bound violations: {viol[:4]}"
    assert st["queries"] >= 8, f"the lazy path ran for {st['queries']} of 16 queries"
    assert st["finite"] >= 0.9 * st["cands"], f"only {st['finite']} of {st['cands']} head blocks have a finite U"
    _HEAD[f"metric {metric} bits {bits} D {dim} x{scale:g}"] = st
    print(f"head bound metric {metric} bits {bits} D {dim} x{scale:g}: {st['finite']}/{st['cands']} finite U over "
          f"{st['queries']} queries, median U / max(dist, lb) = {st['median_ratio']:.3f}")


def _crafted(kind):
    """'ex6_dist': 7-bit L2 index whose 1-bit f_rescale is scaled by 1e-2, so that the refined-distance side of block_ub
    dominates (terms 4, 5 can bite); 'neg_ferr': 1-bit index in which every 7th vector has f_error = -200, so that the
    lower bound exceeds the estimate (term 3 can bite)."""
    data, built = _head_index(0, 7 if kind == "ex6_dist" else 1, 128, 1.0)
    host = pb.host_index_of(built)
    built.close()
    D = int(host.padded_dim)
    s = pb.record_stride(D)
    for cl in host.clusters:
        n = len(cl["ids"])
        for b in range((n + 31) // 32):
            f = cl["batch_data"][b * s + D * 4:(b + 1) * s].view(F32)  # f_add[32] | f_rescale[32] | f_error[32]
            if kind == "ex6_dist":
                f[32:64] *= F32(1e-2)
            else:
                f[64:96][np.arange(32) % 7 == 3] = F32(-200.0)
    return data, host


@pytest.mark.parametrize("kind,required", [("ex6_dist", (0, 1, 4, 5)), ("neg_ferr", (0, 1, 2, 3))])
def test_every_slack_term_is_required_by_the_head_bound_check(env, kind, required):
    """Each rounding-slack term of block_ub scaled to a large negative multiple (options slack_term / slack_milli) must make
    check_head_ub report violations on an index where its side of the bound dominates; at x 1 none is reported."""
    data, host = _crafted(kind)
    idx = rq.IvfRabitqIndex.load_from_bytes(host.rbq1())
    try:
        viol, st = _head_check(env, idx, host, data, kind)
        assert not viol, f"{kind} at x 1: {viol[:4]}"
        assert st["queries"] >= 8
        for term in required:
            idx.set_option("slack_term", term)
            fired = 0
            for milli in (-3_000_000, -300_000_000, -2_000_000_000):  # x -3e3, -3e5, -2e6 of the term
                idx.set_option("slack_milli", milli)
                fired = len(_head_check(env, idx, host, data, kind)[0])
                if fired:
                    break
            idx.set_option("slack_milli", 1000)
            assert fired, f"{kind}: term {term} ({SLACK_TERMS[term]}) scaled negative left every head bound above the vectors"
            _HEAD[f"{kind} term {term} scaled"] = f"{fired} violations"
        assert not _head_check(env, idx, host, data, kind)[0]
    finally:
        idx.close()
