"""Queries in f16 / bf16 (option "query_dtype") on an MI355X.  The contract: ids, counts, score bits, diag, list
outputs and errors of a call with 16-bit queries equal those of the same call with the option at f32 on the rows widened to f32.
Every base case first holds the 16-bit call against the CPU oracle on the widened rows (oracle.search_batch, tests/range_ref.py,
tests/mstg_search_cases.py), then against the library's own f32 call, bit for bit.  Queries are drawn f32 and rounded once, here,
by rerank_f16_ref.round_to; some rows then get planted elements: f16 rows +0, -0, the largest and the smallest subnormal, the
smallest normal and 65504; bf16 rows values up to 2^20.  Deterministic and seeded."""
import functools

import numpy as np
import pytest

import mstg_search_cases as mc
import oracle
import rabitq_rs_amd as rq
import range_ref
from conftest import build_index, make_dataset
from rabitq_rs_amd import RabitqError, _abi
from rerank_f16_ref import BF16, F16, round_to, widen
from rerank_pool_ref import rerank_pool

pytestmark = pytest.mark.gpu

DTYPES = (F16, BF16)
N, NLIST = 4000, 16
MASK = {"native_avx512": 0, "native_avx2": 1, "portable": 6}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def rows16(q32, dtype, seed=0):
    """(bit patterns [nq][dim] u16, their widened f32 values) of f32 queries rounded once, rows 1 and 2 (where they exist) with
    planted elements at seeded positions"""
    bits = round_to(q32, dtype).copy()
    nq, dim = bits.shape
    rng = np.random.default_rng(9000 + seed + dim)
    if dtype == F16:  # +0, -0, the largest / smallest subnormal, the smallest normal | 65504
        plant = [np.array([0x0000, 0x8000, 0x03FF, 0x0001, 0x0400], np.uint16), np.array([0x7BFF], np.uint16)]
    else:             # 2^20, -2^19, 2^10 + 2^3 (bf16 keeps eight bits) | 2^20
        plant = [round_to(np.array([2.0 ** 20, -(2.0 ** 19), 1032.0], np.float32), BF16), round_to(np.array([2.0 ** 20], np.float32), BF16)]
    for row, vals in zip((1, 2), plant):
        if row < nq:
            pos = rng.permutation(dim)[:min(len(vals), dim)]
            bits[row, pos] = vals[:len(pos)]
    return bits, widen(bits, dtype)


def pinned(a):
    """a page-locked copy of a NumPy array (and the tensor that owns it)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int16 if a.dtype == np.uint16 else a.dtype)).pin_memory()
    return t.numpy().view(a.dtype), t


def same(got, want, what=""):
    """ids, score bits (padding included), counts and diag"""
    assert np.array_equal(got[2], want[2]), f"{what}: counts differ at {np.nonzero(got[2] != want[2])[0][:8]}"
    bad = np.nonzero((got[0] != want[0]).any(axis=1))[0]
    assert bad.size == 0, f"{what}: ids differ for queries {bad[:8]}: {got[0][bad[0]][:8]} expected {want[0][bad[0]][:8]}"
    sbad = np.nonzero((_bits(got[1]) != _bits(want[1])).any(axis=1))[0]
    assert sbad.size == 0, f"{what}: score bits differ for queries {sbad[:8]}"
    if len(got) > 3 and got[3] is not None:
        assert want[3] is not None and np.array_equal(got[3], want[3]), f"{what}: SearchDiagnostics differ"


def oracle_topk(built, qw, top_k, nprobe, fw=None, nbits=0, mask=0):
    """the oracle's answer in the library's shape, every distance finite (the widened rows must leave it so)"""
    with oracle.variant(mask):
        rc, ids, sc, cnt, dg = oracle.search_batch(built, qw, top_k, nprobe, fw, nbits, want_diag=True)
    assert rc == 0
    valid = np.arange(top_k)[None, :] < cnt[:, None]
    assert np.isfinite(sc[valid]).all(), "the planted elements left a distance that is not finite"
    return ids, sc, cnt, dg, valid


def against_oracle(got, ref, what=""):
    ids, sc, cnt, dg, valid = ref
    assert np.array_equal(got[2], cnt), f"{what}: counts differ from the oracle's"
    bad = np.nonzero((got[0] != ids).any(axis=1))[0]
    assert bad.size == 0, f"{what}: ids differ from the oracle's for queries {bad[:8]}"
    assert not ((_bits(got[1]) != _bits(sc)) & valid).any(), f"{what}: score bits differ from the oracle's"
    assert np.isnan(got[1][~valid]).all()
    if got[3] is not None:
        assert np.array_equal(got[3], dg), f"{what}: SearchDiagnostics differ from the oracle's"


@functools.lru_cache(maxsize=None)
def case(metric, bits, dim, rot=1, n=N, nlist=NLIST):
    data, built = build_index(n=n, dim=dim, nlist=nlist, total_bits=bits, metric=metric, rotator=rot, normalize=(metric == 1 and dim > 1),
                              seed=3000 + dim + bits)
    return data, built


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    case.cache_clear()
    mstg_case.cache_clear()


def queries(nq, dim, metric, seed=3090):
    return make_dataset(nq, dim, 4, seed + dim, normalize=(metric == 1 and dim > 1))


# ---- 1. preparation outputs: rot, LUT and consts of the three kernels, bitwise against the f32 call -------------------------------
def _prep_outputs(idx, ptr, nq, dim, D, st, top_k=5, nprobe=4):
    import torch
    dev = torch.device("cuda", 0)
    d_i = torch.zeros(nq, top_k, dtype=torch.int64, device=dev)
    d_s = torch.zeros(nq, top_k, dtype=torch.float32, device=dev)
    d_c = torch.zeros(nq, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    idx.search_batch_device(ptr, nq, dim, top_k, nprobe, d_i.data_ptr(), d_s.data_ptr(), d_c.data_ptr(), stream=st.cuda_stream)
    torch.cuda.synchronize(dev)
    Dc = (D + 63) // 64 * 64
    return (idx.debug_copy_workspace(st.cuda_stream, "rot", np.empty((nq, D), np.float32)).view(np.uint32),
            idx.debug_copy_workspace(st.cuda_stream, "lut", np.empty((nq, Dc * 4), np.uint8)),
            idx.debug_copy_workspace(st.cuda_stream, "consts", np.empty((nq, 12), np.float32)).view(np.uint32),
            d_i.cpu().numpy(), _bits(d_s.cpu().numpy()), d_c.cpu().numpy())


# Rows that start 4-byte aligned take the paired 32-bit loads of fhtkac_initial_load_pairs, the others (odd dim from the second row
# on, a base offset by one element) one 16-bit load per element; dim 7 (transform shorter than a wave) and the matrix rotator take
# the element loops of rotate_into_lds.  All of them must give the f32 call's bits.
# (kernel, options, nq, offset by one element): which kernel serves the call is the library's rule (api_search.hip), held below by
# the shape of the launch the stage probe reports
PREP_FHT = [("lat_front", {}, 1, False), ("lat_front", {}, 4, True), ("lat_prep", {}, 5, True), ("lat_prep", {}, 64, False),
            ("wave", {}, 600, False), ("wave", {"latency_path": 0}, 3, True), ("wg", {"wg_prep": 1}, 3, True), ("wg", {"wg_prep": 1}, 9, False)]
PREP_MATRIX = [("wg", {}, 1, False), ("wg", {}, 3, True), ("wg", {}, 5, False)]


# (the builder refuses a matrix rotator whose dimension is no multiple of 16, as the crate does: no such index exists at 7 or 100)
# (101: odd and above a wavefront — even rows take the paired loads with the last element loaded alone, odd rows the element loads)
@pytest.mark.parametrize("rot,dim", [(1, 7), (1, 100), (1, 101), (1, 192), (1, 960), (1, 2048), (0, 192), (0, 960), (0, 2048)],
                         ids=lambda v: str(v))
def test_preparation_outputs(rot, dim):
    import torch
    data, built = case(0, 7, dim, rot)
    D = built.padded_dim
    dev = torch.device("cuda", 0)
    idx = rq.IvfRabitqIndex.from_built(built)
    st32, st16 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)  # (a workspace each: the 16-bit call cannot pass on the f32 call's leftovers)
    try:
        for kernel, opts, nq, offset in (PREP_FHT if rot == 1 else PREP_MATRIX):
            q32 = queries(nq, dim, 0, seed=3100 + nq)
            for k, v in opts.items():
                idx.set_option(k, v)
            for dtype in DTYPES:
                what = f"{kernel} nq={nq} {dtype} offset={offset}"
                bits, qw = rows16(q32, dtype, seed=nq)
                r = np.stack([oracle.rotate(built, x) for x in qw[:4]])
                assert np.isfinite(r).all() and np.isfinite(r.astype(np.float64) @ r.astype(np.float64).T).all()
                d32 = torch.from_numpy(qw).to(dev)
                want = _prep_outputs(idx, d32.data_ptr(), nq, dim, D, st32)
                assert np.array_equal(want[0][:4], r.view(np.uint32)), f"{what}: the f32 call's rotation is not the oracle's"
                # rows of an odd dim start 2-byte aligned only from the second on; `offset` moves the base itself by one element
                flat = torch.zeros(nq * dim + 1, dtype=torch.int16, device=dev)
                flat[int(offset):int(offset) + nq * dim] = torch.from_numpy(bits.view(np.int16).reshape(-1)).to(dev)
                ptr = flat.data_ptr() + 2 * int(offset)
                assert not offset or dim % 2 == 0 or ptr % 4 == 2
                idx.set_query_dtype(dtype)
                try:
                    res = idx.stage_resources(nq, 5, 4)["prep"]
                    got = _prep_outputs(idx, ptr, nq, dim, D, st16)
                finally:
                    idx.set_query_dtype(None)
                for name, g, w in zip(("rot", "lut", "consts", "ids", "score bits", "counts"), got, want):
                    assert np.array_equal(g, w), f"{what}: {name} differs from the f32 call's"
                lists = (NLIST + 31) // 32
                wgs = {"lat_front": (lists + 1 + 7) // 8 * 8 * nq, "lat_prep": nq, "wave": (nq + 3) // 4, "wg": nq}[kernel]
                assert res["workgroups"] == wgs and res["scratch_bytes"] == 0, (what, res)
            for k in opts:
                idx.set_option(k, {"latency_path": 1, "wg_prep": 0}[k])
    finally:
        idx.release_stream(st32.cuda_stream)
        idx.release_stream(st16.cuda_stream)
        idx.close()


# ---- 2. end to end on IVF ---------------------------------------------------------------------------------------------------------
def _host(idx, q, top_k, nprobe, dtype=None, fw=None, nbits=0, diag=True):
    return idx.batch_search_raw(q, rq.SearchParams(top_k, nprobe), fw, nbits, want_diag=diag, dtype=dtype)


@pytest.mark.parametrize("dim", [64, 100, 960])
@pytest.mark.parametrize("bits", [1, 3, 7])
@pytest.mark.parametrize("metric", [0, 1])
def test_host_entry(metric, bits, dim):
    """pageable and page-locked queries, 8 and 600 per call (both inside the zero-copy window), host_zero_copy on and off"""
    data, built = case(metric, bits, dim)
    top_k, nprobe = 10, 5
    q32 = queries(600, dim, metric)
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        for dtype in DTYPES:
            b600, w600 = rows16(q32, dtype)
            ref600 = oracle_topk(built, w600, top_k, nprobe)
            for nq in (8, 600):
                bits16, qw = b600[:nq], np.ascontiguousarray(w600[:nq])
                ref = tuple(x[:nq] for x in ref600)
                want = _host(idx, qw, top_k, nprobe)
                against_oracle(want, ref, f"f32 nq={nq}")
                pin16, keep = pinned(bits16)
                for zc in (1, 0):
                    idx.set_option("host_zero_copy", zc)
                    for name, arr in (("pageable", np.ascontiguousarray(bits16)), ("page-locked", pin16)):
                        what = f"{dtype} nq={nq} {name} zero_copy={zc}"
                        got = _host(idx, arr, top_k, nprobe, dtype)
                        against_oracle(got, ref, what)
                        same(got, want, what)
                idx.set_option("host_zero_copy", 1)
                del keep
        assert idx.query_dtype() == "f32"
    finally:
        idx.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sub_batches_lanes_and_helpers(dtype):
    """300 queries in sub-batches of 64 (the last one 44): with a wrong byte offset a sub-batch reads another query's row.  dim 960:
    the 16-bit call is large enough (512 KiB) for the staging helpers"""
    metric, bits, dim, top_k, nprobe = 0, 7, 960, 10, 5
    data, built = case(metric, bits, dim)
    bits16, qw = rows16(queries(300, dim, metric, seed=3200), dtype)
    assert bits16.nbytes >= 512 << 10
    ref = oracle_topk(built, qw, top_k, nprobe)
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        idx.set_option("host_subbatch", 64)
        want = _host(idx, qw, top_k, nprobe)
        against_oracle(want, ref, "f32")
        pin16, keep = pinned(bits16)
        for lanes in (0, 2):
            for helpers in (1, 0):
                for zc in (1, 0):
                    idx.set_option("host_lanes", lanes)
                    idx.set_option("host_stage_helpers", helpers)
                    idx.set_option("host_zero_copy", zc)
                    for name, arr in (("pageable", bits16), ("page-locked", pin16)):
                        got = _host(idx, arr, top_k, nprobe, dtype)
                        what = f"lanes={lanes} helpers={helpers} zero_copy={zc} {name}"
                        against_oracle(got, ref, what)
                        same(got, want, what)
    finally:
        idx.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_replicas_and_device_entry(dtype):
    import torch
    metric, bits, dim, top_k, nprobe = 1, 3, 100, 10, 5
    data, built = case(metric, bits, dim)
    nq = 301  # (not divisible by the replica count: shards of 150 and 151)
    bits16, qw = rows16(queries(nq, dim, metric, seed=3300), dtype)
    ref = oracle_topk(built, qw, top_k, nprobe)
    one = rq.IvfRabitqIndex.from_built(built)
    two = rq.IvfRabitqIndex.from_built(built, devices=[0, 0])
    try:
        assert two.device_count() == 2
        want = _host(one, qw, top_k, nprobe)
        against_oracle(want, ref, "f32")
        got = _host(two, bits16, top_k, nprobe, dtype)
        against_oracle(got, ref, "two replicas")
        same(got, want, "two replicas")
        same(_host(two, qw, top_k, nprobe), want, "two replicas, f32")
        assert two.query_dtype() == "f32"
        # the device entry on a caller's stream, raw pointers: set_query_dtype
        dev = torch.device("cuda", 0)
        qd = torch.from_numpy(bits16.view(np.int16)).to(dev)
        d_i = torch.zeros(nq, top_k, dtype=torch.int64, device=dev)
        d_s = torch.zeros(nq, top_k, dtype=torch.float32, device=dev)
        d_c = torch.zeros(nq, dtype=torch.int32, device=dev)
        d_d = torch.zeros(nq, 3, dtype=torch.int64, device=dev)
        st = torch.cuda.Stream(dev)
        torch.cuda.synchronize(dev)
        one.set_query_dtype(dtype)
        assert one.query_dtype() == dtype
        one.search_batch_device(qd.data_ptr(), nq, dim, top_k, nprobe, d_i.data_ptr(), d_s.data_ptr(), d_c.data_ptr(), stream=st.cuda_stream,
                                d_diag=d_d.data_ptr())
        torch.cuda.synchronize(dev)
        one.set_query_dtype("f32")
        one.release_stream(st.cuda_stream)
        got = (d_i.cpu().numpy().view(np.uint64), d_s.cpu().numpy(), d_c.cpu().numpy().view(np.uint32), d_d.cpu().numpy().view(np.uint64))
        against_oracle(got, ref, "device entry")
        same(got, want, "device entry")
    finally:
        one.close()
        two.close()


def _words(allowed, nbits):
    w = np.zeros((nbits + 31) // 32 or 1, np.uint32)
    a = np.asarray(sorted(allowed), np.uint64)
    np.bitwise_or.at(w, (a >> np.uint64(5)).astype(np.int64), (np.uint32(1) << (a & np.uint64(31)).astype(np.uint32)))
    return w


@pytest.mark.parametrize("dtype", DTYPES)
def test_filter_diag_and_numeric_variants(dtype):
    metric, bits, dim, top_k, nprobe = 0, 7, 100, 10, 6
    data, built = case(metric, bits, dim)
    bits16, qw = rows16(queries(40, dim, metric, seed=3400), dtype)
    fw = _words(set(range(0, N, 3)), N)
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        for variant in ("native_avx512", "native_avx2", "portable"):
            idx.set_numeric_variant(variant)
            for f, nb in ((None, 0), (fw, N)):
                ref = oracle_topk(built, qw, top_k, nprobe, f, nb, MASK[variant])
                for diag in (True, False):
                    want = _host(idx, qw, top_k, nprobe, None, f, nb, diag)
                    got = _host(idx, bits16, top_k, nprobe, dtype, f, nb, diag)
                    what = f"{variant} filter={f is not None} diag={diag}"
                    against_oracle(got, ref, what)
                    same(got, want, what)
    finally:
        idx.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_range_search(dtype):
    """one radius, rows of a capacity that truncates some queries and not others"""
    metric, bits, dim, nprobe = 0, 7, 100, 6
    data, built = case(metric, bits, dim)
    bits16, qw = rows16(queries(12, dim, metric, seed=3500), dtype)
    r = range_ref.kth_distance_radius(built, qw[0], 30, nprobe)
    ref = range_ref.range_batch(built, qw, r, nprobe)
    tot = np.array([len(x[0]) for x in ref])
    assert all(np.isfinite(x[1]).all() for x in ref)
    cap = int(np.sort(tot)[len(tot) // 2]) or 1
    assert (tot > cap).any() and (tot <= cap).any(), tot
    eids, ebits, etot = range_ref.rows(ref, cap)
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        idx.set_range_search(r)
        want = _host(idx, qw, cap, nprobe)
        got = _host(idx, bits16, cap, nprobe, dtype)
        idx.set_range_search(None)
        assert np.array_equal(got[2], etot) and np.array_equal(got[0], eids) and np.array_equal(_bits(got[1]), ebits)
        assert np.array_equal(got[3], range_ref.diag_of(ref))
        same(got, want, "range")
        # the wrapper: sets both options for the call, puts both back
        lims, ids, sc = idx.range_search(bits16, r, nprobe, dtype=dtype)
        lims32, ids32, sc32 = idx.range_search(qw, r, nprobe)
        assert np.array_equal(lims, lims32) and np.array_equal(ids, ids32) and np.array_equal(_bits(sc), _bits(sc32))
        assert np.array_equal(np.diff(lims), tot) and idx.query_dtype() == "f32"
    finally:
        idx.close()


@pytest.mark.parametrize("raw_dtype", ["f32", "f16"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rerank(dtype, raw_dtype):
    """without a pool (k_rerank) and with pool 32 (k_rerank_pool), over raw rows of f32 and f16; odd and even dim"""
    metric, bits, top_k, nprobe = 0, 3, 10, 6
    for dim in (100, 7):
        data, built = case(metric, bits, dim) if dim == 100 else case(0, 7, 7)
        bits16, qw = rows16(queries(20, dim, metric, seed=3600), dtype)
        raw = data.astype(np.float16) if raw_dtype == "f16" else data
        wide = raw.astype(np.float32)
        idx = rq.IvfRabitqIndex.from_built(built)
        try:
            idx.set_rerank_vectors(raw)
            assert idx.rerank_dtype() == raw_dtype
            idx.set_option("rerank", 0)
            for pool in (0, 32):
                pid, psc, pcnt, _ = _host(idx, qw, max(pool, top_k), nprobe, diag=False)  # the plain search: the pool
                against_oracle((pid, psc, pcnt, None), oracle_topk(built, qw, max(pool, top_k), nprobe), "pool")
                eids, ebits, ecnt = rerank_pool(qw, wide, pid, pcnt, metric, top_k)
                assert np.isfinite(ebits.view(np.float32)[np.arange(top_k)[None, :] < ecnt[:, None]]).all()
                idx.set_option("rerank", 1)
                idx.set_rerank_pool(pool)
                want = _host(idx, qw, top_k, nprobe, diag=False)
                got = _host(idx, bits16, top_k, nprobe, dtype, diag=False)
                idx.set_rerank_pool(0)
                idx.set_option("rerank", 0)
                valid = np.arange(top_k)[None, :] < ecnt[:, None]
                assert np.array_equal(got[2], ecnt) and np.array_equal(got[0][valid], eids[valid]), f"dim {dim} pool {pool}: ids"
                assert np.array_equal(_bits(got[1])[valid], ebits[valid]), f"dim {dim} pool {pool}: exact score bits"
                same(got, want, f"dim {dim} pool {pool}")
        finally:
            idx.close()


# ---- 3. MSTG: posting_scan, the search on host and device buffers, several chunks, the refined search -------------------------------
@functools.lru_cache(maxsize=None)
def mstg_case(metric, bits, dim, nq):
    return mc.kmeans_case(metric, bits, dim, 6000, 48, nq, 61 + dim)


@pytest.mark.parametrize("dim", [64, 112])  # (an MSTG index needs a multiple of 16)
@pytest.mark.parametrize("dtype", DTYPES)
def test_mstg(dtype, dim):
    import torch
    metric, bits, nq, top_k, ef, eps = 0, 7 if dim == 64 else 3, 200, 10, 20, 0.6
    built, cent, q32 = mstg_case(metric, bits, dim, nq)
    bits16, qw = rows16(q32, dtype)
    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        # the f32 call on the widened rows against select_lists_cpu, the oracle's scan and rbq_posting_scan_batch (mc.check)
        want = mc.check(idx, built, cent, qw, top_k, ef, eps, metric)
        assert np.isfinite(want[1][np.arange(top_k)[None, :] < want[2][:, None]]).all()
        rl, rc = want[3], want[4]
        # posting_scan with 16-bit rows: first against the oracle's scan itself, compared as mc.check compares (the reference does not
        # define which of several equal distances is returned, nor the sign of a zero L2 distance), then against the f32 call
        r, oids, osc, ocnt = oracle.posting_scan_batch(built, qw, top_k, rl, rc)
        got = idx.posting_scan(bits16, top_k, rl, rc, dtype=dtype)
        assert r == 0 and np.array_equal(got[2], ocnt)
        mask = np.uint32(0x7fffffff if metric == 0 else 0xffffffff)
        for i in range(nq):
            c = int(ocnt[i])
            s16 = got[1][i, :c]
            assert np.array_equal(_bits(s16) & mask, _bits(osc[i, :c]) & mask), f"posting_scan: score bits of query {i} differ from the oracle's"
            assert (got[0][i, c:] == mc.NONE64).all() and np.isnan(got[1][i, c:]).all()
            if c:
                uniq = np.ones(c, bool)
                uniq[1:] &= s16[1:] != s16[:-1]
                uniq[:-1] &= s16[:-1] != s16[1:]
                uniq &= s16 != s16[-1]
                assert np.array_equal(got[0][i, :c][uniq], oids[i, :c][uniq]), f"posting_scan: ids of query {i} differ from the oracle's"
        same(got, idx.posting_scan(qw, top_k, rl, rc), "posting_scan")

        def lists_too(out, what):
            same(out[:3], want[:3], what)
            assert np.array_equal(out[3], want[3]) and np.array_equal(out[4], want[4]), f"{what}: list outputs differ"

        lists_too(rq.mstg_search(idx, bits16, top_k, ef, eps, return_lists=True, dtype=dtype), "host entry")
        idx.set_option("mstg_search_budget", 1 << 19)  # several chunks of the 200 queries
        lists_too(rq.mstg_search(idx, bits16, top_k, ef, eps, return_lists=True, dtype=dtype), "host entry in chunks")
        dev = torch.device("cuda", 0)
        # (one element into a larger tensor: the rows start 2-byte aligned only)
        flat = torch.zeros(nq * dim + 1, dtype=torch.int16, device=dev)
        flat[1:] = torch.from_numpy(bits16.view(np.int16).reshape(-1)).to(dev)
        t16 = flat[1:].view(nq, dim).view(torch.float16 if dtype == F16 else torch.bfloat16)
        assert t16.data_ptr() % 4 == 2
        for what in ("device entry in chunks", "device entry"):
            out = rq.mstg_search(idx, t16, top_k, ef, eps, return_lists=True)
            torch.cuda.synchronize(dev)
            lists_too((out[0].cpu().numpy().view(np.uint64), out[1].cpu().numpy(), out[2].cpu().numpy().view(np.uint32),
                       out[3].cpu().numpy().view(np.uint32), out[4].cpu().numpy().view(np.uint32)), what)
            idx.set_option("mstg_search_budget", 0)
        if bits > 1:  # the refined search keeps the handle's ex_bits in the preparation
            for budget in (0, 1 << 19):
                idx.set_option("mstg_search_budget", budget)
                w = rq.mstg_search(idx, qw, top_k, ef, eps, return_lists=True, refine_pool=64)
                lists_ok = np.array_equal(w[3], want[3]) and np.array_equal(w[4], want[4])
                assert lists_ok
                g = rq.mstg_search(idx, bits16, top_k, ef, eps, return_lists=True, refine_pool=64, dtype=dtype)
                same(g[:3], w[:3], f"refined, budget {budget}")
                assert np.array_equal(g[3], w[3]) and np.array_equal(g[4], w[4])
                out = rq.mstg_search(idx, t16, top_k, ef, eps, refine_pool=64)
                torch.cuda.synchronize(dev)
                same((out[0].cpu().numpy().view(np.uint64), out[1].cpu().numpy(), out[2].cpu().numpy().view(np.uint32)), w[:3],
                     f"refined device entry, budget {budget}")
            idx.set_option("mstg_search_budget", 0)
        assert idx.query_dtype() == "f32"
    finally:
        idx.close()


# ---- 4. the option ----------------------------------------------------------------------------------------------------------------
def test_option_values_read_back_and_alignment():
    import torch
    data, built = case(0, 7, 100)
    L = rq.index.lib()
    idx = rq.IvfRabitqIndex.from_built(built)
    two = rq.IvfRabitqIndex.from_built(built, devices=[0, 0])
    try:
        v = np.full(1, -1, np.int32)
        for h in (idx, two):
            assert h.query_dtype() == "f32"
            for name, code in (("f16", 1), ("bf16", 2), ("f32", 0), ("bf16", 2)):
                h.set_query_dtype(name)
                assert h.query_dtype() == name
                assert L.rbq_debug_copy_index(h._h, b"query_dtype", v.ctypes.data, 4) == 0 and v[0] == code
            for bad in (3, -1, 16, 1 << 20):  # refused, detail names the three, the previous value stays
                assert L.rbq_debug_set_option(h._h, b"query_dtype", bad) == _abi.RBQ_INVALID_CONFIG
                d = rq.index._detail()
                assert "RBQ_RAW_F32" in d and "RBQ_RAW_F16" in d and "RBQ_RAW_BF16" in d and str(bad) in d
                assert h.query_dtype() == "bf16"
            assert L.rbq_debug_copy_index(h._h, b"query_dtype", v.ctypes.data, 8) == _abi.RBQ_INVALID_CONFIG
            with pytest.raises(RabitqError):
                h.set_query_dtype("f64")
            assert h.query_dtype() == "bf16"
            h.set_query_dtype(None)
        # an odd pointer: refused while the option is 16-bit (before anything is launched), accepted as ever at f32
        nq, dim, top_k = 4, 100, 5
        buf = np.zeros(nq * dim * 4 + 8, np.uint8)
        odd = buf.ctypes.data + (1 if buf.ctypes.data % 2 == 0 else 2)
        ids, sc, cnt = np.zeros((nq, top_k), np.uint64), np.zeros((nq, top_k), np.float32), np.full(nq, 77, np.uint32)
        dev = torch.device("cuda", 0)
        dbuf = torch.zeros(nq * dim * 4 + 8, dtype=torch.uint8, device=dev)
        d_i = torch.zeros(nq, top_k, dtype=torch.int64, device=dev)
        d_s = torch.zeros(nq, top_k, dtype=torch.float32, device=dev)
        d_c = torch.full((nq,), 77, dtype=torch.int32, device=dev)
        for h in (idx, two):
            cnt[:] = 77
            for name in ("f16", "bf16"):
                h.set_query_dtype(name)
                assert L.rbq_search_batch(h._h, odd, nq, dim, top_k, 4, None, 0, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, None) == _abi.RBQ_INVALID_CONFIG
                assert rq.index._detail() == "queries: pointer not aligned to its 16-bit elements"
                assert L.rbq_search_batch_device(h._h, dbuf.data_ptr() + 1, nq, dim, top_k, 4, None, 0, d_i.data_ptr(), d_s.data_ptr(), d_c.data_ptr(),
                                                 None, None) == _abi.RBQ_INVALID_CONFIG
                assert rq.index._detail() == "queries: pointer not aligned to its 16-bit elements"
                # the earlier checks keep their order and their texts
                assert L.rbq_search_batch(h._h, odd, nq, dim + 1, top_k, 4, None, 0, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, None) == _abi.RBQ_DIMENSION_MISMATCH
                assert rq.index._detail() == "expected 100, got 101"
                assert L.rbq_search_batch(h._h, None, nq, dim, top_k, 4, None, 0, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, None) == _abi.RBQ_INVALID_CONFIG
                assert rq.index._detail() == "null buffer"
            h.set_query_dtype("f32")
            assert (cnt == 77).all()
            torch.cuda.synchronize(dev)
            assert (d_c.cpu().numpy() == 77).all()
            assert L.rbq_search_batch(h._h, odd, nq, dim, top_k, 4, None, 0, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data, None) == 0
    finally:
        idx.close()
        two.close()


def test_wrappers_restore_the_handle():
    import torch
    metric, dim, top_k, nprobe = 0, 100, 10, 5
    data, built = case(metric, 7, dim)
    q32 = queries(9, dim, metric, seed=3700)
    idx = rq.IvfRabitqIndex.from_built(built)
    never = rq.IvfRabitqIndex.from_built(built)  # a handle whose option is never set
    try:
        p = rq.SearchParams(top_k, nprobe)
        base = never.batch_search_raw(q32, p, want_diag=True)
        against_oracle(base, oracle_topk(built, q32, top_k, nprobe), "f32, option never set")
        idx.set_option("query_dtype", 0)
        same(idx.batch_search_raw(q32, p, want_diag=True), base, "option explicitly 0")
        for dtype in DTYPES:
            b16, qw = rows16(q32, dtype)
            want = never.batch_search_raw(qw, p, want_diag=True)
            for before in ("f32", "bf16", "f16"):  # whatever set_query_dtype left on the handle comes back, after success ...
                idx.set_query_dtype(before)
                same(idx.batch_search_raw(b16, p, want_diag=True, dtype=dtype), want, f"{dtype} on a handle at {before}")
                assert idx.query_dtype() == before
                same(idx.batch_search_raw(qw, p, want_diag=True), want, f"f32 input on a handle at {before}")
                assert idx.query_dtype() == before
                with pytest.raises(RabitqError) as e:  # ... and after a raised error (the library's own dimension check)
                    idx.batch_search_raw(b16[:, :dim - 1], p, dtype=dtype)
                assert e.value.code == _abi.RBQ_DIMENSION_MISMATCH and idx.query_dtype() == before
            # the option set directly, not through set_query_dtype: the wrappers go by what the handle holds
            idx.set_option("query_dtype", _abi.RAW_F16)
            same(idx.batch_search_raw(qw, p, want_diag=True), want, "f32 input after a direct set_option")
            assert idx.query_dtype() == "f16"
            same(idx.batch_search_raw(b16, p, want_diag=True, dtype=dtype), want, f"{dtype} after a direct set_option")
            assert idx.query_dtype() == "f16"
            idx.set_query_dtype(None)
            # every array-taking wrapper, against its f32 form
            r16, r32 = idx.search(b16[0], p, dtype=dtype), never.search(qw[0], p)
            assert [(x.id, x.score) for x in r16] == [(x.id, x.score) for x in r32] and len(r16) == top_k
            r16, r32 = idx.search_filtered(b16[1], p, range(0, N, 2), dtype=dtype), never.search_filtered(qw[1], p, range(0, N, 2))
            assert [(x.id, x.score) for x in r16] == [(x.id, x.score) for x in r32] and len(r16) > 0
            r16, r32 = idx.batch_search(b16, p, dtype=dtype), never.batch_search(qw, p)
            assert [[(x.id, x.score) for x in r] for r in r16] == [[(x.id, x.score) for x in r] for r in r32]
            for a, b in zip(idx.batch_query(b16, top_k, nprobe, dtype=dtype), never.batch_query(qw, top_k, nprobe)):
                assert np.array_equal(_bits(a), _bits(b))
            assert idx.query_dtype() == "f32"
            # the inputs the marshalling accepts without `dtype`
            with pytest.raises(RabitqError) as e:
                idx.batch_search_raw(b16, p)
            assert e.value.code == _abi.RBQ_INVALID_CONFIG and "uint16" in str(e.value) and idx.query_dtype() == "f32"
            tt = torch.float16 if dtype == F16 else torch.bfloat16
            host_t = torch.from_numpy(b16.view(np.int16)).view(tt)
            same(idx.batch_search_raw(host_t, p, want_diag=True), want, f"{dtype} host tensor")
            dev_t = host_t.to(torch.device("cuda", 0))
            same(idx.batch_search_raw(dev_t, p, want_diag=True), want, f"{dtype} device tensor")
            if dtype == F16:
                same(idx.batch_search_raw(b16.view(np.float16), p, want_diag=True), want, "numpy.float16 array")
            assert idx.query_dtype() == "f32"
        same(idx.batch_search_raw(torch.from_numpy(q32).to(torch.device("cuda", 0)), p, want_diag=True), base, "f32 device tensor")
    finally:
        idx.close()
        never.close()
