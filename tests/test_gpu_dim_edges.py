"""Every GPU path at the dimension edges: trunc 1-8 (dim 1-15, padded to 64), odd dims around multiples of 64, D = 2048 on the Kac
path (trunc 1024) and as a power of two (rotate_fhtkac_wave<32>), and the Matrix rotator at 16, 80, 1008 and 2048.  Search (every
route), stage outputs, the heap's LDS / global-memory crossover at D = 2048, the device encoders, k-means, brute force, fetch, save
and rerank, each against the existing reference of that operation; and the refusal of dim 2049 on every creation path.
The oracle's rotation at these dims is checked against a float64 restatement in tests/test_dim_edges_host.py."""
import ctypes as C

import numpy as np
import pytest

import oracle
import rabitq_rs_amd as rq
from conftest import build_index, make_dataset
from rabitq_rs_amd import _abi
from rabitq_rs_amd.index import lib
from rabitq_rs_amd.kmeans import KMeansConfig, first_draw
from rescale_ref import crafted_rows, normalize_rows
from test_dim_edges_host import KAC_DIMS, MATRIX_DIMS, TOO_WIDE
from test_gpu_bruteforce import check as bf_check, make as bf_make
from test_gpu_encode_optimal import _bits, _same_index
from test_gpu_fetch import _bits_equal, _check_index, _dataset as _fetch_dataset
from test_gpu_kmeans import _run_both
from test_gpu_latency import test_latency_front_stage_outputs as _latency_stage_outputs
from test_gpu_numeric_variant import _compare
from test_gpu_save import _same as _save_same, _stream_build as _save_stream_build
from test_gpu_round2 import test_stage_level_parity as _stage_level_parity

pytestmark = pytest.mark.gpu

NATIVE = "native_avx512"  # the default numeric variant; _compare checks ids, counts, diagnostics and score BITS under it
TINY = [d for d in KAC_DIMS if d < 16]
# (dim, rotator, total_bits, metric): L2 at 7 bits and IP at 3 bits everywhere; 1 bit for trunc < 16 and for 2048
SEARCH = ([(d, 1, 7, 0) for d in KAC_DIMS] + [(d, 1, 3, 1) for d in KAC_DIMS] + [(d, 1, 1, 0) for d in TINY + [2048]] +
          [(d, 0, 7, 0) for d in MATRIX_DIMS] + [(d, 0, 3, 1) for d in MATRIX_DIMS])


def _sid(case):
    d, rot, bits, metric = case
    return f"{'kac' if rot else 'matrix'}_d{d}_{bits}bit_{'IP' if metric else 'L2'}"


def _index(dim, rot, bits, metric, n=600, nlist=6, faster=True):
    data, built = build_index(n=n, dim=dim, nlist=nlist, total_bits=bits, metric=metric, rotator=rot, normalize=(metric == 1),
                              seed=7000 + dim + bits, faster=faster)
    return data, built, rq.IvfRabitqIndex.from_built(built)


def _queries(nq, dim, metric, seed):
    return make_dataset(nq, dim, 2, seed, normalize=(metric == 1))


def _words(allowed, nbits):
    words = np.zeros((nbits + 31) // 32, np.uint32)
    np.bitwise_or.at(words, allowed >> 5, (np.uint32(1) << (allowed & 31).astype(np.uint32)))
    return words


# ---- 2. search against the oracle, every route ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SEARCH, ids=_sid)
def test_search_routes_match_oracle(case):
    dim, rot, bits, metric = case
    data, built, idx = _index(dim, rot, bits, metric)
    q40 = _queries(40, dim, metric, 7100 + dim)
    top_k, nprobe = 10, 3
    outs = []
    for sw in (0, 1):  # batch path, k_scan / k_scanw
        idx.set_option("scan_wave", sw)
        outs.append(_compare(built, idx, q40, top_k, nprobe, NATIVE))
    idx.set_option("scan_wave", -1)
    for opt in ("latency_path", "wg_prep"):  # k_prep_wave (one wave per query) / k_prep with a workgroup per query
        idx.set_option(opt, 1 if opt == "wg_prep" else 0)
        outs.append(_compare(built, idx, q40, top_k, nprobe, NATIVE))
        idx.set_option(opt, 0 if opt == "wg_prep" else 1)
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(_bits(o[1]), _bits(outs[0][1]))
    for nq in (1, 4, 5, 200):  # latency front (1, 4); the workgroup-per-query preparation of the batch path (5 .. 512)
        q = _queries(nq, dim, metric, 7200 + nq)
        _compare(built, idx, q, top_k, nprobe, NATIVE)
    _compare(built, idx, data[:8], top_k, 6, NATIVE)  # exact hits (at dims 1 and 2: heavy ties, the tie log and the heap emulation)
    if dim == 2048 and rot == 1:
        for ks in (2, 4):
            idx.set_option("rank_ksplit", ks)
            _compare(built, idx, q40, top_k, nprobe, NATIVE)
        idx.set_option("rank_ksplit", 1)
    if dim in (1, 33, 2048):
        allowed = np.arange(0, data.shape[0], 3)
        words = _words(allowed, data.shape[0])
        ids, _, cnt = _compare(built, idx, q40, top_k, nprobe, NATIVE, filter_words=words, filter_nbits=data.shape[0])
        assert set(ids[np.arange(top_k)[None, :] < cnt[:, None]].tolist()) <= set(allowed.tolist())
        res = idx.search_filtered(q40[0], rq.SearchParams(top_k, nprobe), allowed.tolist())
        assert [r.id for r in res] == ids[0, :cnt[0]].tolist()
    if dim in (33, 2048) and bits > 1:
        _compare(built, idx, q40, top_k, nprobe, "portable")
        _compare(built, idx, q40[:4], top_k, nprobe, "portable")
        idx.set_numeric_variant(NATIVE)
    idx.close()


@pytest.mark.parametrize("dim", [1, 33, 1025, 2048])
@pytest.mark.parametrize("metric,bits", [(0, 7), (1, 3)])
def test_stage_outputs_bit_for_bit(dim, metric, bits):
    """rotated query, LUT bytes, delta, sum_vl, the query constants and the probe list against the oracle's stage functions (batch
    path: test_stage_level_parity; latency front: test_latency_front_stage_outputs, scores of every list)"""
    _stage_level_parity(600, dim, 6, bits, metric, 1, 24, 4, False, True)
    _latency_stage_outputs(600, dim, 6, bits, metric, 3)


# ---- 3. the heap's crossover from LDS to global memory ---------------------------------------------------------------------------
def _crossover(idx, nq, nprobe):
    """smallest top_k whose scan heap leaves the LDS: above 256 the LDS heap takes (top_k + 1) * 8 bytes of the scan's LDS"""
    lds = lambda k: idx.stage_resources(nq, k, nprobe)["scan"]["lds_bytes"]  # noqa: E731
    base = lds(257) - 258 * 8
    in_lds = lambda k: lds(k) == base + (k + 1) * 8  # noqa: E731
    lo, hi = 257, 1 << 20
    assert in_lds(lo) and not in_lds(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if in_lds(mid) else (lo, mid)
    return hi


@pytest.mark.parametrize("dim", [2048, 64])
def test_heap_crossover_at_d2048(dim):
    """The smallest top_k whose heap leaves the LDS, from the library's own launch plan: kTopKMax + 1 = 16385 at D = 64, and at
    D = 2048 with ex 6 too (measured: the 160 KB of a gfx950 workgroup still hold the 16384-entry heap beside the D = 2048 query).
    Search at crossover - 1, crossover and crossover + 1 equals the oracle's, with more candidates than top_k (the heap evicts)."""
    nq, nprobe = 3, 2
    n = 18500 if dim == 2048 else 17500
    data, built = build_index(n=n, dim=dim, nlist=2, total_bits=7, seed=7300 + dim)
    idx = rq.IvfRabitqIndex.from_built(built)
    x = _crossover(idx, nq, nprobe)
    assert x == 16385
    assert n > x + 1000
    q = _queries(nq, dim, 0, 7301)
    for k in (x - 1, x, x + 1):
        ids, sc, cnt = _compare(built, idx, q, k, nprobe, NATIVE)
        assert (cnt == k).all()
    idx.close()


# ---- 4. device build paths against the CPU builder, array for array -----------------------------------------------------------
BUILD = [(d, 1) for d in KAC_DIMS] + [(d, 0) for d in MATRIX_DIMS]


@pytest.mark.parametrize("dim,rot", BUILD, ids=[f"{'kac' if r else 'matrix'}_d{d}" for d, r in BUILD])
def test_device_builds_match_cpu_builder(dim, rot):
    import torch
    n, nlist, bits, metric = 300, 4, 7, 0
    data = make_dataset(n, dim, 2, 7400 + dim)
    cent, assign = rq.builder.kmeans(data, nlist, 3, 7401)
    xd = torch.from_numpy(data).cuda()
    ad = torch.from_numpy(assign.astype(np.int32)).cuda()
    for faster in (True, False):
        built = rq.builder.train_with_clusters(data, cent, assign, bits, metric, rot, 7402, faster)
        ref = rq.IvfRabitqIndex.from_built(built)
        one = rq.IvfRabitqIndex.build_on_device(built.hdr_ptr, cent, xd.data_ptr(), ad.data_ptr(), n,
                                                built.t_const if faster else None, rescale="const" if faster else "optimal")
        _same_index(ref, one, built.hdr, nlist)
        sb = rq.StreamBuilder(built.hdr_ptr, cent, np.bincount(assign, minlength=nlist), built.t_const if faster else None,
                              rescale="const" if faster else "optimal")
        for a, b in ((0, 1), (1, 97), (97, 98), (98, n)):  # ragged pushes
            sb.push(data[a:b], assign[a:b], a)
        streamed = sb.finish()
        _same_index(ref, streamed, built.hdr, nlist)
        trained = rq.IvfRabitqIndex.train_on_device(data, cent, assign, bits, metric, rot, 7402, faster)
        _same_index(ref, trained, built.hdr, nlist)
        if not faster:
            _compare(built, one, _queries(8, dim, metric, 7403), 10, 2, NATIVE)
        for x in (one, streamed, trained, ref, built):
            x.close()


@pytest.mark.parametrize("ex_bits", [2, 6])
@pytest.mark.parametrize("dim", [1, 3, 33, 1025, 2047])
def test_device_best_rescale_at_edge_dims(dim, ex_bits):
    import rescale_ref
    rows = [o for _, o in crafted_rows(dim, 7500 + dim + ex_bits)]
    rng = np.random.default_rng(dim + ex_bits)
    O = np.concatenate([np.stack(rows), normalize_rows(rng.standard_normal((300 if dim > 1000 else 2000, dim)))])
    got = rq.IvfRabitqIndex.debug_best_rescale(O, ex_bits)
    want = np.array([rescale_ref.best_rescale_factor(o, ex_bits) for o in O[:40]] +
                    [rq.builder.best_rescale_factor(o, ex_bits) for o in O[40:]])
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert bad.size == 0, f"{bad.size} rows differ, first {bad[:5]}"


# ---- 5. device k-means, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2, 3, 31, 32, 33, 65, 2048])
def test_device_kmeans_at_edge_dims(dim):
    data = make_dataset(500 if dim < 2048 else 300, dim, 3, 7600 + dim)
    _run_both(data, 8, KMeansConfig(niter=5, seed=dim))


@pytest.mark.parametrize("n,k,cfg", [(200, 1, KMeansConfig(niter=3, seed=1)), (60, 60, KMeansConfig(niter=3, seed=2)),
                                     (400, 6, KMeansConfig(niter=5, seed=3, spherical=True))], ids=["k1", "k_eq_n", "spherical"])
def test_device_kmeans_odd_dim_corners(n, k, cfg):
    _run_both(make_dataset(n, 33, 3, 7700 + k, normalize=cfg.spherical), k, cfg)


def test_device_kmeans_dim_2049_matches():
    """k-means has no dimension limit in the crate, and none here: dim 2049 (Dp = 2080) matches the CPU restatement bit for bit"""
    _run_both(make_dataset(200, 2049, 3, 7800), 5, KMeansConfig(niter=3, seed=4))


@pytest.mark.parametrize("dim", [3, 2047])
def test_train_end_to_end_at_edge_dims(dim):
    n, nlist, bits, seed = 400, 4, 7, 7900 + dim
    data = make_dataset(n, dim, 2, seed)
    km = rq.builder.run_kmeans_with_config_cpu(data, nlist, KMeansConfig(niter=30, seed=first_draw(seed ^ 0x5A5A5A5A5A5A5A5A)))
    built = rq.builder.train_with_clusters(data, km.centroids, km.assignments, bits, 0, 1, seed, False)
    ref = rq.IvfRabitqIndex.from_built(built)
    idx = rq.IvfRabitqIndex.train(data, nlist, bits, 0, rq.RotatorType.FhtKacRotator, seed, False)
    _same_index(ref, idx, built.hdr, nlist)
    _compare(built, idx, _queries(8, dim, 0, seed), 10, 2, NATIVE)
    ref.close(); idx.close()


# ---- 6. brute force --------------------------------------------------------------------------------------------------------
BF = [(d, 1) for d in (1, 7, 33, 100, 1025, 2048)] + [(2048, 0)]


@pytest.mark.parametrize("dim,rot", BF, ids=[f"{'kac' if r else 'matrix'}_d{d}" for d, r in BF])
@pytest.mark.parametrize("bits,metric", [(7, 0), (3, 1), (1, 0)])
def test_bruteforce_at_edge_dims(dim, rot, bits, metric):
    n = 150 if dim >= 1025 else 400
    data, built, idx, prep = bf_make(n, dim, bits, metric, rot, 8000 + dim + bits, dup=20)
    q = np.random.default_rng(dim).standard_normal((5, dim)).astype(np.float32)
    bf_check(idx, prep, q, 10)
    bf_check(idx, prep, q[:2], n + 7)  # top_k above n
    bf_check(idx, prep, data[:3], 5)
    if dim == 33 and bits > 1:  # (a trained 1-bit index's RBF1 carries ex bytes its reader does not read: the crate refuses it too)
        blob = idx.save_to_bytes()
        back = rq.BruteForceRabitqIndex.load_from_bytes(blob)
        assert back.save_to_bytes() == blob
        bf_check(back, prep, q, 10)
        back.close()
    idx.close()


# ---- 7. fetch and save -----------------------------------------------------------------------------------------------------
# every creation path over test_gpu_save's crafted clustering (empty lists, lists of 1, 31, 32, 33, 65 and 300 vectors).  The device
# inputs are held in named tensors for the whole build: a temporary's data_ptr() is freed (and may be handed to the next upload by
# the caching allocator) before the call it is passed to runs.
def _creation_paths(built, cent, data, assign, faster):
    import torch
    xd = torch.from_numpy(data).cuda()
    ad = torch.from_numpy(assign.astype(np.int32)).cuda()
    yield "from_built", rq.IvfRabitqIndex.from_built(built)
    yield "load_from_bytes", rq.IvfRabitqIndex.load_from_bytes(built.save_rbq1())
    yield "build_on_device", rq.IvfRabitqIndex.build_on_device(built.hdr_ptr, cent, xd.data_ptr(), ad.data_ptr(), data.shape[0],
                                                               built.t_const if faster else None,
                                                               rescale="const" if faster else "optimal")
    yield "StreamBuilder", _save_stream_build(built, cent, data, assign, faster)


@pytest.mark.parametrize("dim", [1, 7, 33, 1025, 2048])
@pytest.mark.parametrize("bits", [7, 3, 1])
def test_fetch_at_edge_dims(dim, bits):
    import torch
    rng = np.random.default_rng(8100 + dim + bits)
    data, cent, assign = _fetch_dataset(dim, 0, 8100 + dim)
    for faster in ((True, False) if bits > 1 else (True,)):
        built = rq.builder.train_with_clusters(data, cent, assign, bits, 0, 1, 8101, faster)
        stream = built.save_rbq1()
        for name, idx in _creation_paths(built, cent, data, assign, faster):
            q, want, wfound = _check_index(idx, f"d{dim} {name} faster={faster}", rng, stream)  # host entry against fetch_ref
            d_ids = torch.from_numpy(q.view(np.int64)).cuda()
            d_out = torch.full((q.size, dim), 7.0, dtype=torch.float32, device="cuda")
            d_found = torch.full((q.size,), 9, dtype=torch.uint8, device="cuda")
            s = torch.cuda.Stream()
            torch.cuda.synchronize()
            idx.fetch_embeddings_device(d_ids.data_ptr(), q.size, d_out.data_ptr(), d_found.data_ptr(), s.cuda_stream)
            s.synchronize()
            _bits_equal(d_out.cpu().numpy(), want, f"device entry, {name}")
            assert np.array_equal(d_found.cpu().numpy().astype(bool), wfound)
            idx.close()
        built.close()


@pytest.mark.parametrize("dim", [1, 33, 2047])
@pytest.mark.parametrize("bits", [7, 3, 1])
def test_save_at_edge_dims(dim, bits):
    """every creation path saves the CPU writer's RBQ1 stream byte for byte, and the reloaded index answers identically"""
    data, cent, assign = _fetch_dataset(dim, 0, 8200 + dim)
    q = _queries(24, dim, 0, 8202)
    for faster in ((True, False) if bits > 1 else (True,)):
        built = rq.builder.train_with_clusters(data, cent, assign, bits, 0, 1, 8201, faster)
        want = built.save_rbq1()
        for name, idx in _creation_paths(built, cent, data, assign, faster):
            _save_same(idx.save_to_bytes(), want, f"d{dim} {name} faster={faster}")
            back = rq.IvfRabitqIndex.load_from_bytes(want)
            ra, rb = idx.batch_search_raw(q, rq.SearchParams(10, 4)), back.batch_search_raw(q, rq.SearchParams(10, 4))
            assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[2], rb[2]) and np.array_equal(_bits(ra[1]), _bits(rb[1]))
            _compare(built, idx, q, 10, 4, NATIVE)
            back.close(); idx.close()
        built.close()


# ---- 8. rerank -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [33, 2048])
@pytest.mark.parametrize("metric", [0, 1])
def test_rerank_at_edge_dims(dim, metric):
    import torch
    data, built, idx = _index(dim, 1, 7, metric)
    L = oracle.lib()
    idx.set_rerank_vectors(data)
    for nq in (1, 40):
        q = _queries(nq, dim, metric, 8300 + nq)
        rc, oids, _, ocnt, _ = oracle.search_batch(built, q, 20, 4)
        dev = torch.device("cuda", 0)
        qd = torch.from_numpy(q).to(dev)
        d_ids = torch.zeros(nq, 20, dtype=torch.int64, device=dev)
        d_sc = torch.zeros(nq, 20, dtype=torch.float32, device=dev)
        d_cnt = torch.zeros(nq, dtype=torch.int32, device=dev)
        st = torch.cuda.Stream(dev)
        torch.cuda.synchronize(dev)
        idx.search_batch_device(qd.data_ptr(), nq, dim, 20, 4, d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr(), stream=st.cuda_stream)
        torch.cuda.synchronize(dev)
        host = idx.batch_search_raw(q, rq.SearchParams(20, 4))
        device = (d_ids.cpu().numpy().view(np.uint64), d_sc.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32))
        for rid, rsc, rcnt in (host[:3], device):
            assert np.array_equal(rcnt, ocnt)
            for i in range(nq):
                c = int(rcnt[i])
                assert sorted(rid[i, :c].tolist()) == sorted(oids[i, :c].tolist())
                exact = np.array([(L.ref_l2_distance_sqr if metric == 0 else L.ref_dot)(q[i].ctypes.data, data[int(j)].ctypes.data, dim)
                                  for j in rid[i, :c]], np.float32)
                assert np.array_equal(exact.view(np.uint32), rsc[i, :c].view(np.uint32))
                assert (np.diff(rsc[i, :c]) >= 0).all() if metric == 0 else (np.diff(rsc[i, :c]) <= 0).all()
        idx.release_stream(st.cuda_stream)
    idx.close()


# ---- 9. dim 2049 is refused on every creation path ----------------------------------------------------------------------------
def _refused(e, kinds=("InvalidConfig",)):
    assert e.value.kind in kinds and e.value.detail, (e.value.kind, e.value.detail)


def test_dim_2049_refused_on_every_creation_path():
    import torch
    n, dim, nlist = 40, 2049, 2
    data, built = build_index(n=n, dim=dim, nlist=nlist, total_bits=7, seed=8400)
    assert built.padded_dim == 2112
    h = C.c_void_p()
    assert lib().rbq_index_create(C.cast(built.hdr_ptr, C.c_void_p), C.cast(built.lists_ptr, C.c_void_p), 1, None, C.byref(h)) == \
        _abi.RBQ_INVALID_CONFIG and h.value is None
    for make in (rq.IvfRabitqIndex.from_built, rq.IvfRabitqIndex.from_built_without_recon):
        with pytest.raises(rq.RabitqError) as e:
            make(built)
        assert e.value.detail == TOO_WIDE
    blob = built.save_rbq1()
    buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
    assert lib().rbq_index_load_rbq1(buf, len(blob), 1, None, C.byref(h)) in (_abi.RBQ_INVALID_CONFIG, _abi.RBQ_INVALID_PERSISTENCE)
    assert h.value is None
    with pytest.raises(rq.RabitqError) as e:
        rq.IvfRabitqIndex.load_from_bytes(blob)
    _refused(e, ("InvalidConfig", "InvalidPersistence"))
    cent = np.stack([built.centroid(c)[:dim] for c in range(nlist)])
    xd = torch.from_numpy(data).cuda()
    _, assign = rq.builder.kmeans(data, nlist, 2, 1)
    ad = torch.from_numpy(assign.astype(np.int32)).cuda()
    for mode, t in ((_abi.RESCALE_MODES["const"], built.t_const), (_abi.RESCALE_MODES["optimal"], 0.0)):
        rc = lib().rbq_index_build_device_ex(C.cast(built.hdr_ptr, C.c_void_p), cent.ctypes.data, C.c_void_p(xd.data_ptr()),
                                             C.c_void_p(ad.data_ptr()), n, mode, t, 0, C.addressof(h))
        assert rc == _abi.RBQ_INVALID_CONFIG and h.value is None
    with pytest.raises(rq.RabitqError) as e:
        rq.IvfRabitqIndex.build_on_device(built.hdr_ptr, cent, xd.data_ptr(), ad.data_ptr(), n, built.t_const)
    _refused(e)
    with pytest.raises(rq.RabitqError) as e:
        rq.StreamBuilder(built.hdr_ptr, cent, np.bincount(assign, minlength=nlist), built.t_const)
    _refused(e)
    with pytest.raises(rq.RabitqError) as e:
        rq.IvfRabitqIndex.train_on_device(data, cent, assign, 7, 0, 1, 8400, True)
    _refused(e)
    with pytest.raises(rq.RabitqError) as e:
        rq.IvfRabitqIndex.train(data, nlist, 7, 0, 1, 8400, True)
    _refused(e)
    with pytest.raises(rq.RabitqError) as e:
        rq.IvfRabitqIndex.debug_best_rescale(np.zeros((1, dim), np.float32), 6)
    _refused(e)
    bb = rq.builder.train_bruteforce(data, 7, 0, 1, 8401, True)
    from rabitq_rs_amd import bruteforce as bfm
    assert bfm.lib().rbq_bf_create(C.cast(bb.hdr_ptr, C.c_void_p), C.cast(bb.view_ptr, C.c_void_p), -1, C.byref(h)) == \
        _abi.RBQ_INVALID_CONFIG and h.value is None
    with pytest.raises(rq.RabitqError) as e:
        rq.BruteForceRabitqIndex.from_built(bb)
    assert e.value.kind == "InvalidConfig" and e.value.detail == TOO_WIDE
    hd, a = bb.header, bb.arrays()
    from rbf1_writer import write_rbf1
    rbf = write_rbf1(hd.dim, hd.padded_dim, hd.metric, hd.rotator, hd.ex_bits, bb.rotator_blob(), a["bin"], a["ex"], a)
    with pytest.raises(rq.RabitqError) as e:
        rq.BruteForceRabitqIndex.load_from_bytes(rbf)
    _refused(e, ("InvalidConfig", "InvalidPersistence"))
