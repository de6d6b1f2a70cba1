"""MSTG posting-list build on the GPU (include/rbq_mstg.h): device closure assignment equals the CPU restatement exactly, its
shortlist holds every centroid the exact order needs, and build_postings_on_device equals the CPU builder over the expanded
(vector, list) pairs byte for byte, posting scans included."""
import numpy as np
import pytest
import torch

import closure_cases as cc
import closure_ref
import rabitq_rs_amd as rq
from rabitq_rs_amd import _abi, mstg

pytestmark = pytest.mark.gpu

NONE64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _same(x, c, eps, m, **kw):
    want = rq.closure_assign_cpu(x, c, eps, m)
    got = rq.closure_assign(x, c, eps, m, **kw)
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0], want[0])


@pytest.mark.parametrize("case", range(len(cc.CRATE_UNIT)))
def test_the_crates_own_unit_test_inputs(case):
    eps, m, v, c = cc.CRATE_UNIT[case]
    _same(np.asarray(v, np.float32), np.asarray(c, np.float32), eps, m)


def test_main_case():
    x, c, eps, m = cc.main_case()
    _same(x, c, eps, m)


def test_default_epsilon_case():
    x, c, eps, m = cc.default_epsilon_case()
    _same(x, c, eps, m)


@pytest.mark.parametrize("name", sorted(cc.shortlist_dim_cases()))
def test_shortlist_path_at_odd_dims(name):
    """more than 256 centroids at dims 7, 9 and 100: k_km_split's zero padding to a multiple of 32 under k_cl_scan, and the
    tail coordinates of the 8-lane canonical distance"""
    x, c = cc.shortlist_dim_cases()[name]
    before = mstg.closure_fallbacks()
    for eps in cc.EPSILONS:
        for m in cc.REPLICAS:
            _same(x, c, eps, m, max_chunk_rows=200)
    fallbacks = mstg.closure_fallbacks() - before
    print(name, "fallback rows", fallbacks, "of", 16 * len(x))
    assert fallbacks < 16 * len(x)
    st = {}
    closure_ref.closure_assign(x, c, 0.15, 8, st)
    sl, sl_n = mstg.debug_closure_shortlist(x, c, 8)
    for i, order in enumerate(st["order"]):
        if sl_n[i] != mstg.NONE:
            assert set(order) <= set(int(v) for v in sl[i, :sl_n[i]]), (i, order)


@pytest.mark.parametrize("name", sorted(cc.dim_cases()))
def test_dims_and_list_counts(name):
    x, c = cc.dim_cases()[name]
    for eps in cc.EPSILONS:
        for m in cc.REPLICAS:
            _same(x, c, eps, m)


@pytest.mark.parametrize("name", sorted(cc.tie_cases()))
def test_ties(name):
    x, c = cc.tie_cases()[name]
    for eps in cc.EPSILONS:
        for m in cc.REPLICAS:
            _same(x, c, eps, m)


@pytest.fixture(scope="module")
def large():
    """dim 960, 1024 centroids: the GEMM shortlist path"""
    return cc.clustered(3000, 960, 1024, 77)


def test_large_case_uses_the_shortlist_host_and_device_input_and_chunks(large):
    x, c = large
    want = rq.closure_assign_cpu(x, c, 0.15, 8)
    before = mstg.closure_fallbacks()
    got = rq.closure_assign(x, c, 0.15, 8)
    fallbacks = mstg.closure_fallbacks() - before
    print("fallback rows", fallbacks, "of", len(x), "replication", want[1].mean())
    assert fallbacks < len(x)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()
    for kw in ({}, {"max_chunk_rows": 700}, {"max_chunk_rows": 129}):
        got = rq.closure_assign(xd, cd, 0.15, 8, **kw)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    got = rq.closure_assign(x, cd, 2.0, 16, max_chunk_rows=1000)
    want = rq.closure_assign_cpu(x, c, 2.0, 16)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_duplicated_centroids_through_the_shortlist():
    """1200 centroids, every one twice: ties at every rank, cut included"""
    x, c = cc.clustered(1500, 64, 600, 21)
    c2 = np.concatenate([c, c]).astype(np.float32)
    for eps, m in ((0.15, 8), (10.0, 3), (2.0, 1), (0.0, 16)):
        _same(x, c2, eps, m)
    x[:50] = c[:50]
    _same(x, c2, 0.15, 8, max_chunk_rows=333)


def test_a_common_offset_falls_back_and_still_matches():
    """data + 300: every centroid is within 2 eps of every other, so rows fall back to all 400 centroids"""
    x, c = cc.clustered(600, 40, 400, 31)
    x, c = (x + 300.0).astype(np.float32), (c + 300.0).astype(np.float32)
    before = mstg.closure_fallbacks()
    _same(x, c, 0.15, 8)
    assert mstg.closure_fallbacks() - before > 0


def test_shortlist_holds_the_first_max_replicas_of_the_exact_order(large):
    x, c = large
    x = x[:700]
    for m in (8, 16):
        st = {}
        closure_ref.closure_assign(x, c, 0.15, m, st)
        sl, sl_n = mstg.debug_closure_shortlist(x, c, m)
        checked = 0
        for i, order in enumerate(st["order"]):
            if sl_n[i] == mstg.NONE:
                continue
            assert m <= sl_n[i] <= 256
            row = sl[i, :sl_n[i]]
            assert (np.diff(row.astype(np.int64)) > 0).all()
            assert set(order) <= set(int(v) for v in row), (i, order, row)
            checked += 1
        assert checked > len(x) // 2


def test_non_finite_input_is_invalid_config():
    x, c = cc.clustered(300, 32, 300, 41)
    x[17, 3] = np.inf
    with pytest.raises(rq.RabitqError) as e:
        rq.closure_assign(x, c, 0.15, 8)
    assert e.value.code == _abi.RBQ_INVALID_CONFIG and "finite" in e.value.detail


def _arrays(idx, hdr, nlist):
    D, ex = hdr.padded_dim, hdr.ex_bits
    Dc = (D + 63) // 64 * 64
    ln = idx.debug_copy_index("list_n", np.empty(nlist, np.uint32))
    nblocks = int(((ln + 31) // 32).sum())
    cpu_u = 128 // ex if ex else 1
    w4 = ((D // 16 + cpu_u - 1) // cpu_u) if ex else 0
    sizes = {"list_gb0": nlist * 4, "list_n": nlist * 4, "centroids": nlist * D * 4, "blocks": nblocks * (Dc * 4 + 384),
             "ids": nblocks * 32 * 8, "bsum": nblocks * 32, "delta": nblocks * 32 * 4, "vl": nblocks * 32 * 4,
             "cent_hi": nlist * D * 2, "cent_lo": nlist * D * 2, "cnorm2": nlist * 4}
    if ex:
        sizes.update({"ex": nblocks * 32 * w4 * 256, "fadd_ex": nblocks * 32 * 4, "fres_ex": nblocks * 32 * 4})
    return {name: idx.debug_copy_index(name, np.empty(nbytes, np.uint8)) for name, nbytes in sizes.items()}


@pytest.mark.parametrize("bits", [1, 3, 7])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("faster", [True, False])
def test_build_equals_the_cpu_builder_over_the_expanded_pairs(bits, metric, faster):
    n, dim, k, eps, m = 1500, 64, 24, 2.0, 8
    x, c = cc.clustered(n, dim, k, 300 + bits)
    lists, counts = rq.closure_assign_cpu(x, c, eps, m)
    pair_vec, pair_list = mstg.expand_pairs(lists, counts)
    assert len(pair_vec) > 1.2 * n
    built = rq.builder.train_with_clusters(x[pair_vec], c, pair_list, bits, metric, rq.RotatorType.NoRotation, 42, faster)
    ref = rq.IvfRabitqIndex.from_built(built)
    for data, kw in ((x, {}), (torch.from_numpy(x).cuda(), {"max_chunk_rows": 401})):
        dev = rq.build_postings_on_device(data, c, bits, metric, closure_epsilon=eps, max_replicas=m, faster_config=faster, **kw)
        assert len(dev) == len(ref) == len(pair_vec) and dev.cluster_count() == k
        a, b = _arrays(ref, built.header, k), _arrays(dev, built.header, k)
        for name in a:
            if name == "ids":
                ia, ib = a[name].view(np.uint64), b[name].view(np.uint64)
                real = ia != NONE64
                assert np.array_equal(real, ib != NONE64)
                assert np.array_equal(pair_vec[ia[real].astype(np.int64)].astype(np.uint64), ib[real])
            else:
                bad = np.nonzero(a[name] != b[name])[0]
                assert bad.size == 0, f"{name}: {bad.size} bytes differ, first at {bad[:5]}"
        rng = np.random.default_rng(5)
        q = (x[rng.integers(0, n, 48)] + 0.01 * rng.standard_normal((48, dim))).astype(np.float32)
        lc = rng.integers(0, 7, 48).astype(np.uint32)
        lc[0] = 0
        li = np.stack([rng.permutation(k)[:6] for _ in range(48)]).astype(np.uint32)
        ra, rb = ref.posting_scan(q, 10, li, lc), dev.posting_scan(q, 10, li, lc)
        assert np.array_equal(ra[2], rb[2])
        for i in range(48):
            cnt = int(ra[2][i])
            assert np.array_equal(pair_vec[ra[0][i, :cnt].astype(np.int64)].astype(np.uint64), rb[0][i, :cnt])
            assert np.array_equal(ra[1][i, :cnt].view(np.uint32), rb[1][i, :cnt].view(np.uint32))
        # boundaries of a RBQ_ROTATOR_NONE handle, as before
        for fn, msg in ((dev.save_to_bytes, "posting-list handles (RBQ_ROTATOR_NONE) have no RBQ1 rotator tag and cannot be saved"),
                        (lambda: dev.fetch_embeddings([0, 1]), "posting-list handles (RBQ_ROTATOR_NONE) have no rotator to invert")):
            with pytest.raises(rq.RabitqError) as e:
                fn()
            assert e.value.code == _abi.RBQ_INVALID_CONFIG and e.value.detail == msg
        outs = []
        for h in (ref, dev):
            try:
                ids, sc, cn, _ = h.batch_search_raw(q[:8], rq.SearchParams(5, 4))
                outs.append(("ok", cn.tolist(), sc.view(np.uint32).tolist()))
            except rq.RabitqError as e:
                outs.append((e.code, e.detail))
        assert outs[0] == outs[1]
        dev.close()
    ref.close()
    built.close()
