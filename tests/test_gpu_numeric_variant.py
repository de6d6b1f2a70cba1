"""The numeric variant switch (rbq_index_set_numeric_variant): which build of the reference the kernels reproduce bit for bit.
Every comparison is against the oracle under the matching mask (oracle/rbq_ref.c, "Numeric variants"): native_avx2 = mask 1
(ex_avx2), portable = mask 6 (ex_scalar + epilogue_scalar).  Ids, counts and SearchDiagnostics are equal and the scores are equal
BIT FOR BIT, with and without diagnostics.  Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest

import oracle
import rabitq_rs_amd as rq
from conftest import build_index, make_dataset

pytestmark = pytest.mark.gpu

MASK = {"native_avx512": 0, "native_avx2": 1, "portable": 6}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _compare(built, idx, queries, top_k, nprobe, variant, mask=None, filter_words=None, filter_nbits=0):
    """GPU under `variant` against the oracle under its mask: ids, counts, diagnostics, score bits; then the same call without
    diagnostics must return the same bits"""
    mask = MASK[variant] if mask is None else mask
    idx.set_numeric_variant(variant)
    with oracle.variant(mask):
        rc, oids, osc, ocnt, odiag = oracle.search_batch(built, queries, top_k, nprobe, filter_words, filter_nbits, want_diag=True)
    assert rc == 0
    ids, sc, cnt, diag = idx.batch_search_raw(queries, rq.SearchParams(top_k, nprobe), filter_words, filter_nbits, want_diag=True)
    assert np.array_equal(cnt, ocnt), f"counts differ: {np.nonzero(cnt != ocnt)[0][:10]}"
    bad = np.nonzero((ids != oids).any(axis=1))[0]
    assert bad.size == 0, f"ids differ for queries {bad[:10]}: gpu={ids[bad[0]]} oracle={oids[bad[0]]}"
    valid = np.arange(top_k)[None, :] < cnt[:, None]
    sbad = np.nonzero(((_bits(sc) != _bits(osc)) & valid).any(axis=1))[0]
    assert sbad.size == 0, f"score bits differ for queries {sbad[:10]}: gpu={sc[sbad[0]]} oracle={osc[sbad[0]]}"
    assert np.isnan(sc[~valid]).all()
    assert np.array_equal(diag, odiag), "SearchDiagnostics counters differ"
    ids2, sc2, cnt2, _ = idx.batch_search_raw(queries, rq.SearchParams(top_k, nprobe), filter_words, filter_nbits, want_diag=False)
    assert np.array_equal(cnt2, cnt) and np.array_equal(ids2, ids), "results differ without diagnostics"
    assert np.array_equal(_bits(sc2), _bits(sc)), "scores differ without diagnostics"
    return ids, sc, cnt


SHAPES = [
    # n, dim, nlist, bits, metric, nq, top_k, nprobe
    pytest.param(6000, 128, 48, 7, 0, 32, 10, 12, id="d128_7bit_L2"),
    pytest.param(6000, 128, 48, 3, 1, 32, 10, 12, id="d128_3bit_IP"),
    pytest.param(4000, 128, 32, 1, 0, 32, 10, 8, id="d128_1bit_L2"),
    pytest.param(4000, 128, 32, 1, 1, 32, 10, 8, id="d128_1bit_IP"),
    pytest.param(6000, 960, 48, 7, 0, 24, 10, 12, id="d960_7bit_L2"),
    pytest.param(6000, 960, 48, 3, 1, 24, 10, 16, id="d960_3bit_IP"),
    pytest.param(5000, 768, 40, 7, 1, 24, 10, 10, id="d768_7bit_IP"),
    pytest.param(5000, 768, 40, 3, 0, 24, 10, 10, id="d768_3bit_L2"),
    pytest.param(4000, 100, 32, 7, 0, 32, 10, 8, id="d100_pad128_kac_7bit_L2"),
    pytest.param(1500, 40, 12, 3, 0, 20, 10, 12, id="kac_d40_trunc32_3bit_L2"),
]


@pytest.mark.parametrize("variant", ["native_avx2", "portable"])
@pytest.mark.parametrize("n,dim,nlist,bits,metric,nq,top_k,nprobe", SHAPES)
def test_variant_shapes_match_oracle(n, dim, nlist, bits, metric, nq, top_k, nprobe, variant):
    """Generator queries and queries taken from the data (near-exact hits).  At 1 bit no ex code is evaluated: portable is the
    scalar epilogue alone (oracle mask 4) and native_avx2 is the default's arithmetic."""
    data, built = build_index(n=n, dim=dim, nlist=nlist, total_bits=bits, metric=metric, normalize=(metric == 1), seed=700 + dim + bits)
    idx = rq.IvfRabitqIndex.from_built(built)
    q = np.concatenate([make_dataset(nq, dim, max(nlist // 4, 1), 701 + dim, normalize=(metric == 1)), data[:16] + np.float32(1e-4)])
    q = np.ascontiguousarray(q, dtype=np.float32)
    _compare(built, idx, q, top_k, nprobe, variant)
    if bits == 1:
        _compare(built, idx, q, top_k, nprobe, variant, mask=4 if variant == "portable" else 0)
    idx.close()


def _random_case(seed):  # (the shape generator of test_gpu_parity.test_random_configurations_match_oracle)
    rng = np.random.default_rng(seed)
    rot = int(rng.integers(0, 2))
    dim = int(rng.choice([16, 24, 40, 64, 96, 100, 128, 200, 256, 384, 512, 768])) if rot == 1 else int(rng.choice([16, 32, 48, 64, 96, 128]))
    bits = int(rng.choice([1, 3, 7]))
    metric = int(rng.integers(0, 2))
    nlist = int(rng.integers(2, 60))
    n = int(rng.integers(max(nlist, 40), 4000))
    nq = int(rng.integers(1, 40))
    top_k = int(rng.choice([1, 2, 5, 10, 17, 64, 100]))
    nprobe = int(rng.integers(1, nlist + 3))
    return n, dim, nlist, bits, metric, rot, nq, top_k, nprobe


@pytest.mark.parametrize("seed", list(range(100, 144)))
def test_random_configurations_portable(seed):
    n, dim, nlist, bits, metric, rot, nq, top_k, nprobe = _random_case(seed)
    data, built = build_index(n=n, dim=dim, nlist=nlist, total_bits=bits, metric=metric, rotator=rot, seed=seed, normalize=(metric == 1))
    idx = rq.IvfRabitqIndex.from_built(built)
    q = make_dataset(nq, dim, max(nlist // 4, 1), seed + 1000, normalize=(metric == 1))
    _compare(built, idx, q, top_k, nprobe, "portable")
    idx.close()


@pytest.fixture(scope="module")
def d960():
    data, built = build_index(n=8000, dim=960, nlist=64, total_bits=7, metric=0, seed=733)
    q = np.ascontiguousarray(np.concatenate([make_dataset(40, 960, 16, 734), data[:24] + np.float32(1e-3)]), dtype=np.float32)
    return data, built, q


@pytest.mark.parametrize("scan_wave", [0, 1])
@pytest.mark.parametrize("top_k", [10, 64, 100, 257])
def test_portable_scan_kernels_and_topk_layouts(d960, scan_wave, top_k):
    """k_scan and k_scanw, register-run (10, 64, 100) and LDS-heap (257) top-k layouts"""
    data, built, q = d960
    idx = rq.IvfRabitqIndex.from_built(built)
    idx.set_option("scan_wave", scan_wave)
    _compare(built, idx, q, top_k, 16, "portable")
    idx.close()


@pytest.mark.parametrize("opt,val", [("block_bound", 0), ("block_bound", 1), ("exact_heap", 1), ("lazy_select", 0),
                                     ("latency_path", 0)])
def test_portable_routes(d960, opt, val):
    data, built, q = d960
    idx = rq.IvfRabitqIndex.from_built(built)
    idx.set_option(opt, val)
    _compare(built, idx, q, 10, 16, "portable")
    _compare(built, idx, q, 100, 16, "native_avx2")
    idx.close()


@pytest.mark.parametrize("nq", [1, 4, 8])
def test_portable_latency_path(d960, nq):
    data, built, q = d960
    idx = rq.IvfRabitqIndex.from_built(built)
    idx.set_option("latency_path", 1)
    _compare(built, idx, q[:nq], 10, 16, "portable")
    _compare(built, idx, q[24:24 + nq], 10, 16, "portable")
    idx.close()


def test_portable_filtered_search():
    data, built = build_index(n=6000, dim=128, nlist=32, total_bits=7, seed=741)
    idx = rq.IvfRabitqIndex.from_built(built)
    q = make_dataset(24, 128, 8, 742)
    rng = np.random.default_rng(743)
    allowed = rng.choice(6000, 900, replace=False)
    nbits = int(allowed.max()) + 1
    words = np.zeros((nbits + 31) // 32, np.uint32)
    np.bitwise_or.at(words, allowed >> 5, (np.uint32(1) << (allowed & 31).astype(np.uint32)))
    ids, sc, cnt = _compare(built, idx, q, 10, 16, "portable", filter_words=words, filter_nbits=nbits)
    assert set(ids[cnt[:, None] > np.arange(10)[None, :]].tolist()) <= set(allowed.tolist())
    idx.close()


def test_portable_lazy_select_audit_is_clean():
    """lazy selection on (the default): the lists dropped as a whole are lists whose every vector the reference (under the same
    arithmetic) skipped by the lower bound"""
    import torch
    n, dim = 30000, 960
    data, built = build_index(n=n, dim=dim, nlist=128, total_bits=7, metric=0, seed=751)
    idx = rq.IvfRabitqIndex.from_built(built)
    idx.set_numeric_variant("portable")
    rng = np.random.default_rng(752)
    nq, top_k, nprobe = 32, 10, 48
    q = np.ascontiguousarray(data[rng.choice(n, nq, replace=False)] + 0.05 * rng.standard_normal((nq, dim)).astype(np.float32))
    dev = torch.device("cuda", 0)
    qd = torch.from_numpy(q).to(dev)
    d_ids = torch.zeros(nq, top_k, dtype=torch.int64, device=dev)
    d_sc = torch.zeros(nq, top_k, dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(nq, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    idx.set_option("lazy_audit", 1)
    idx.search_batch_device(qd.data_ptr(), nq, dim, top_k, nprobe, d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr(),
                            stream=st.cuda_stream)
    torch.cuda.synchronize(dev)
    aud = idx.debug_copy_workspace(st.cuda_stream, "audit_dead", np.empty((nq, 1024), np.uint32))
    idx.set_option("lazy_audit", 0)
    idx.release_stream(st.cuda_stream)
    dropped, violations = 0, 0
    with oracle.variant(MASK["portable"]):
        rc, oids, osc, _, _ = oracle.search_batch(built, q, top_k, nprobe)
        for i in range(nq):
            nd = int(aud[i, 0])
            assert nd <= 1023
            dead = set(int(c) for c in aud[i, 1:1 + nd])
            cids, ev = oracle.search_lists(built, q[i], top_k, nprobe, None, 0)
            evaluated = {int(c): int(e) for c, e in zip(cids, ev)}
            dropped += len(dead & set(evaluated))
            violations += sum(evaluated.get(c, 0) for c in dead)
    assert rc == 0
    assert np.array_equal(d_ids.cpu().numpy().view(np.uint64), oids)
    assert np.array_equal(_bits(d_sc.cpu().numpy()), _bits(osc))
    assert dropped > 0 and violations == 0, (dropped, violations)
    idx.close()


def test_portable_duplicates_replay_tie_log():
    base = make_dataset(700, 64, 4, 761)
    data = np.concatenate([base, base, base[:300]], axis=0)
    _, built = build_index(nlist=12, total_bits=7, data=data, dim=64)
    idx = rq.IvfRabitqIndex.from_built(built)
    _compare(built, idx, base[:48], 100, 6, "portable")
    _compare(built, idx, base[:16], 10, 12, "portable")
    assert idx.tie_log_stats()["replays"] > 0
    idx.close()


def test_portable_device_entry():
    import torch
    data, built = build_index(n=20000, dim=128, nlist=96, total_bits=7, seed=771)
    idx = rq.IvfRabitqIndex.from_built(built)
    idx.set_numeric_variant("portable")
    nq, top_k, nprobe = 160, 10, 12
    q = make_dataset(nq, 128, 24, 772)
    dev = torch.device("cuda", 0)
    qd = torch.from_numpy(q).to(dev)
    d_i = torch.empty(nq, top_k, dtype=torch.int64, device=dev)
    d_s = torch.empty(nq, top_k, dtype=torch.float32, device=dev)
    d_c = torch.empty(nq, dtype=torch.int32, device=dev)
    idx.search_batch_device(qd.data_ptr(), nq, 128, top_k, nprobe, d_i.data_ptr(), d_s.data_ptr(), d_c.data_ptr(), stream=None)
    torch.cuda.synchronize(dev)
    with oracle.variant(MASK["portable"]):
        rc, oids, osc, ocnt, _ = oracle.search_batch(built, q, top_k, nprobe)
    assert rc == 0
    assert np.array_equal(d_i.cpu().numpy().view(np.uint64), oids)
    assert np.array_equal(d_c.cpu().numpy().view(np.uint32), ocnt)
    assert np.array_equal(_bits(d_s.cpu().numpy()), _bits(osc))
    idx.close()


@pytest.mark.parametrize("metric,bits", [(0, 7), (1, 3)])
def test_portable_mstg_posting_scan(metric, bits):
    """MSTG posting-list scan (src/mstg/index.rs:296: the same compute_batch_distances_u16): oracle under mask 6"""
    seed = 781
    rng = np.random.default_rng(seed)
    data = make_dataset(6000, 128, 12, seed, normalize=(metric == 1))
    cent, assign = rq.builder.kmeans(data, 48, 5, seed)
    built = rq.builder.train_with_clusters(data, cent, assign, bits, metric, rq.RotatorType.NoRotation, seed, True)
    q = make_dataset(40, 128, 12, seed + 1, normalize=(metric == 1))
    d = ((q[:, None, :] - cent[None, :, :]) ** 2).sum(-1)
    lists = np.ascontiguousarray(np.argsort(d, axis=1).astype(np.uint32)[:, :12])
    counts = rng.integers(1, 13, 40).astype(np.uint32)
    idx = rq.IvfRabitqIndex.from_built(built)
    idx.set_numeric_variant("portable")
    differ = 0
    for top_k in (10, 100):
        with oracle.variant(MASK["portable"]):
            rc, oids, osc, ocnt = oracle.posting_scan_batch(built, q, top_k, lists, counts)
        rc0, _, osc0, _ = oracle.posting_scan_batch(built, q, top_k, lists, counts)
        assert rc == 0 and rc0 == 0
        ids, sc, cnt = idx.posting_scan(q, top_k, lists, counts)
        assert np.array_equal(cnt, ocnt)
        for i in range(len(q)):
            c = int(cnt[i])
            # (the distance sets agree bit for bit; ids wherever the distance is unique — the reference leaves ties unordered)
            assert np.array_equal(np.sort(_bits(sc[i, :c]) & 0x7fffffff), np.sort(_bits(osc[i, :c]) & 0x7fffffff)), i
            uniq = np.ones(c, bool)
            uniq[1:] &= sc[i, 1:c] != sc[i, :c - 1]
            uniq[:-1] &= sc[i, :c - 1] != sc[i, 1:c]
            if c:
                uniq[-1] = False  # (a candidate tied with the last one may sit past the cut)
            assert np.array_equal(ids[i, :c][uniq], oids[i, :c][uniq]), i
            differ += int(not np.array_equal(_bits(osc[i, :c]), _bits(osc0[i, :c])))
    assert differ > 0  # the scalar epilogue does change MSTG distances
    idx.close()


def test_default_unchanged_after_switching_back(d960):
    data, built, q = d960
    fresh = rq.IvfRabitqIndex.from_built(built)
    ids0, sc0, cnt0, d0 = fresh.batch_search_raw(q, rq.SearchParams(10, 16), want_diag=True)
    fresh.close()
    idx = rq.IvfRabitqIndex.from_built(built)
    assert idx.numeric_variant == "native_avx512"
    idx.set_numeric_variant("portable")
    idx.batch_search_raw(q, rq.SearchParams(10, 16))
    idx.set_numeric_variant("native_avx512")
    ids, sc, cnt, d = idx.batch_search_raw(q, rq.SearchParams(10, 16), want_diag=True)
    assert np.array_equal(ids, ids0) and np.array_equal(cnt, cnt0) and np.array_equal(d, d0)
    assert np.array_equal(_bits(sc), _bits(sc0))
    _compare(built, idx, q, 10, 16, "native_avx512")
    idx.close()


def test_switch_changes_score_bits(d960):
    """guards against a switch that is silently ignored: on d960 7-bit L2 most queries' scores differ in their last bits"""
    data, built, q = d960
    idx = rq.IvfRabitqIndex.from_built(built)
    ids0, sc0, cnt0, _ = idx.batch_search_raw(q, rq.SearchParams(10, 16))
    idx.set_numeric_variant("portable")
    ids2, sc2, cnt2, _ = idx.batch_search_raw(q, rq.SearchParams(10, 16))
    differ = np.array([not np.array_equal(_bits(sc0[i, :cnt0[i]]), _bits(sc2[i, :cnt2[i]])) for i in range(len(q))])
    assert differ.mean() >= 0.5, differ.mean()
    idx.close()


def test_bad_values_rejected():
    data, built = build_index(n=2000, dim=64, nlist=8, total_bits=7, seed=791)
    idx = rq.IvfRabitqIndex.from_built(built)
    lib = rq.index.lib()
    for name, v in (("native_avx2", 1), ("portable", 2), ("native_avx512", 0)):
        idx.set_numeric_variant(name)
        assert idx.numeric_variant == name and lib.rbq_index_numeric_variant(idx._h) == v
    idx.set_numeric_variant("portable")
    for v in (-1, 3):
        assert lib.rbq_index_set_numeric_variant(idx._h, v) == rq.index._abi.RBQ_INVALID_CONFIG
        assert "numeric variant" in rq.index._detail()
    assert lib.rbq_debug_set_option(idx._h, b"numeric_variant", 3) == rq.index._abi.RBQ_INVALID_CONFIG
    assert "numeric variant" in rq.index._detail()
    assert idx.numeric_variant == "portable"  # (a rejected value changes nothing)
    assert lib.rbq_debug_set_option(idx._h, b"numeric_variant", 1) == 0 and idx.numeric_variant == "native_avx2"
    with pytest.raises(rq.RabitqError):
        idx.set_numeric_variant("avx9000")
    assert lib.rbq_abi_version() == (2 << 16) | 2
    idx.close()
