"""The exact rerank of the MSTG candidate pool (option "mstg_rerank" on rbq_mstg_search_refined_batch / _device; include/rbq_mstg.h,
DESIGN.md section 35; k_mstg_rerank.hip) on an MI355X.  Every comparison is exact: the selected lists are select_lists_cpu's, and
ids, counts and score bits equal the NumPy restatement tests/mstg_rerank_ref.py, whose pool is mstg_refine_ref's and whose sums are
the oracle's canonical l2_distance_sqr / dot.  Every returned row holds pairwise distinct ids.  Seeded."""
import ctypes as C

import numpy as np
import pytest
import torch

import mstg_file as mf
import mstg_refine_ref as rref
import mstg_rerank_ref as ref
import rabitq_rs_amd as rq
from rabitq_rs_amd import _abi, _marshal, mstg
from rabitq_rs_amd.index import lib

pytestmark = pytest.mark.gpu
NONE64 = ref.NONE64
EF, EPS = 6, 0.6
RAWS = ("f32", "f16", "bf16")


def attach(idx, x, raw, n=None):
    """attach rows of type `raw` (16-bit rows rounded here); returns the rows as the scorer sees them, widened to f32"""
    x = np.ascontiguousarray(x[:n] if n is not None else x, np.float32)
    if raw == "f32":
        idx.set_rerank_vectors(x)
        return x
    if raw == "f16":
        h = x.astype(np.float16)
        idx.set_rerank_vectors(h, dtype="f16")
        return h.astype(np.float32)
    b = ref.round_bf16(x)
    idx.set_rerank_vectors(b, dtype="bf16")
    return ref.widen_bf16(b)


def bits_equal(a, b):
    a, b = (v.cpu().numpy() if torch.is_tensor(v) else v for v in (a, b))
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def compare(got, case, q, lists, counts, raw, top_k, pool, cands=None, pair_vec=None, n_raw=None, wide_queries=None):
    """got = (ids, scores, counts[, lists, list_counts]) of the exact call against the restatement"""
    ids, sc, cnt = got[:3]
    if len(got) > 3:
        assert np.array_equal(got[4], counts) and np.array_equal(got[3], lists)
    pv = case.pair_vec if pair_vec is None else pair_vec
    wi, ws, wc, ties = ref.rerank_ref(case.built, pv, q, lists, counts, raw, case.metric, top_k, pool, cands, n_raw, wide_queries)
    assert not any(ties)  # (an estimate tie at the pool's cut is decided by the scan's heap: the data must not have one)
    assert np.array_equal(cnt, wc), (np.nonzero(cnt != wc)[0][:10], cnt[:10], wc[:10])
    bad = np.nonzero((ids != wi).any(axis=1))[0]
    assert bad.size == 0, (bad[:10], ids[bad[0]], wi[bad[0]])
    for i in range(len(q)):
        c = int(cnt[i])
        assert np.array_equal(sc[i, :c].view(np.uint32), ws[i, :c].view(np.uint32)), (i, sc[i, :c], ws[i, :c])
        assert (ids[i, c:] == NONE64).all() and np.isnan(sc[i, c:]).all(), i
        assert len(set(ids[i, :c].tolist())) == c, i
    return ids, sc, cnt


def run(idx, case, q, raw, top_k, ef, eps, pool, **kw):
    lists, counts = rq.select_lists_cpu(q, case.c, ef, eps)
    got = rq.mstg_search(idx, q, top_k, ef, eps, return_lists=True, refine_pool=pool, exact=True)
    return compare(got, case, q, lists, counts, raw, top_k, pool, **kw)


# ---- 1. the main case ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(b, m) for b in (1, 7) for m in (0, 1)], ids=lambda p: "bits%d_metric%d" % p)
def main(request):
    bits, metric = request.param
    case, q = rref.main_case(bits, metric)
    idx = case.device_index()
    lists, counts = rq.select_lists_cpu(q, case.c, EF, EPS)
    cands = rref.all_candidates(case.built, case.pair_vec, q, lists, counts)
    yield case, q, idx, lists, counts, cands
    idx.close()


@pytest.fixture(scope="module")
def main70():
    """7 bits, L2, f32 rows attached: the handle of the tests that are about the plumbing"""
    case, q = rref.main_case(7, 0)
    idx = case.device_index()
    idx.set_rerank_vectors(case.x)
    want = rq.mstg_search(idx, q, 10, EF, EPS, return_lists=True, refine_pool=40, exact=True)
    yield case, q, idx, want
    idx.close()


@pytest.mark.parametrize("raw", RAWS)
def test_main_case(main, raw):
    case, q, idx, lists, counts, cands = main
    wide = attach(idx, case.x, raw)
    for top_k, pool in ((10, 10), (10, 40), (10, 4096), (100, 40)):
        got = rq.mstg_search(idx, q, top_k, EF, EPS, return_lists=True, refine_pool=pool, exact=True)
        compare(got, case, q, lists, counts, wide, top_k, pool, cands)
    idx.set_rerank_vectors(None)


# ---- 2. dimensions: the spans, the partial last span, the largest LDS footprint -------------------------------------------------
@pytest.mark.parametrize("dim", [16, 48, 960, 2048])
def test_dimensions(dim):
    import closure_cases as cc
    x, c = cc.clustered(300, dim, 8, 500 + dim)
    case = rref.Case(x, c, 7, dim // 16 % 2, 2.0, 8)
    rng = np.random.default_rng(dim)
    q = (x[rng.integers(0, 300, 12)] + 0.01 * rng.standard_normal((12, dim))).astype(np.float32)
    idx = case.device_index()
    lists, counts = rq.select_lists_cpu(q, case.c, 4, EPS)
    cands = rref.all_candidates(case.built, case.pair_vec, q, lists, counts)
    for raw in ("f32", "f16"):
        wide = attach(idx, x, raw)
        for pool in (40, 4096):
            got = rq.mstg_search(idx, q, 10, 4, EPS, return_lists=True, refine_pool=pool, exact=True)
            compare(got, case, q, lists, counts, wide, 10, pool, cands)
    idx.close()


# ---- 3, 4. list lengths, exact ties ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,metric", [(7, 0), (1, 1)])
def test_list_lengths_0_1_32_33(bits, metric):
    case, q = rref.list_length_case(bits, metric)
    idx = rq.IvfRabitqIndex.from_built(case.built_with_real_ids())
    idx.set_rerank_vectors(case.x)
    for pool in (0, 4096):
        ids, sc, cnt = run(idx, case, q, case.x, 10, 4, 1e9, pool)
        assert (cnt == 10).all()
    ids, sc, cnt = run(idx, case, q, case.x, 100, 4, 1e9, 0)
    assert (cnt == 66).all()  # every vector of the index, once
    idx.close()


@pytest.mark.parametrize("bits,metric", [(7, 0), (1, 1)])
def test_exact_ties_are_ordered_by_rank(bits, metric):
    case, q = rref.exact_tie_case(bits, metric)
    idx = rq.IvfRabitqIndex.from_built(case.built_with_real_ids())
    idx.set_rerank_vectors(case.x)
    ids, sc, cnt = run(idx, case, q, case.x, 120, 4, 1e9, 4096)  # pool > candidates: every entry is scored
    assert (cnt == 120).all()
    m = 60
    for i in range(len(q)):
        pos = {int(v): p for p, v in enumerate(ids[i])}
        for v in range(m):  # twins hold one vector: equal exact distances whichever lists hold them, next to each other
            a, b = pos[v], pos[v + m]
            assert sc[i, a].view(np.uint32) == sc[i, b].view(np.uint32) and abs(a - b) == 1, (i, v)
            if v % 2 == 0:  # the same list: equal estimates too, so the earlier vector has the smaller rank
                assert a < b, (i, v)
    run(idx, case, q, case.x, 10, 4, 1e9, 4096)
    idx.close()


# ---- 5, 6. ids without a raw row, non-finite queries ---------------------------------------------------------------------------
def test_ids_at_or_above_n_raw_vanish(main):
    case, q, idx, lists, counts, cands = main
    full = attach(idx, case.x, "f32")
    all_ids, _, all_cnt = rq.mstg_search(idx, q, 10, EF, EPS, refine_pool=4096, exact=True)
    wide = attach(idx, case.x, "f32", n=700)
    got = rq.mstg_search(idx, q, 10, EF, EPS, return_lists=True, refine_pool=4096, exact=True)
    ids, sc, cnt = compare(got, case, q, lists, counts, full, 10, 4096, cands, n_raw=700)
    assert (ids[ids != NONE64] < 700).all() and (all_ids[all_ids != NONE64] >= 700).any()
    attach(idx, case.x, "f32", n=100)                         # a pool of 40 holds fewer than 10 of the first 100 ids
    got = rq.mstg_search(idx, q, 10, EF, EPS, return_lists=True, refine_pool=40, exact=True)
    ids, sc, cnt40 = compare(got, case, q, lists, counts, full, 10, 40, cands, n_raw=100)
    assert (all_cnt == 10).all() and (cnt40 < 10).all()       # counts drop
    attach(idx, case.x, "f16", n=1)                           # a single row: only id 0 can stay
    got = rq.mstg_search(idx, q, 10, EF, EPS, return_lists=True, refine_pool=4096, exact=True)
    ids, sc, cnt = compare(got, case, q, lists, counts, case.x[:1].astype(np.float16).astype(np.float32), 10, 4096, cands, n_raw=1)
    assert (cnt <= 1).all() and (cnt == 0).any()
    idx.set_rerank_vectors(None)


def test_non_finite_queries_select_nothing(main70):
    case, q, idx, _ = main70
    q = q[:6].copy()
    q[1, 5] = np.nan
    q[4, :] = np.inf
    ids, sc, cnt = run(idx, case, q, case.x, 10, EF, EPS, 40)
    assert cnt[1] == 0 and cnt[4] == 0 and (cnt[[0, 2, 3, 5]] > 0).all()


# ---- 7. 16-bit queries -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qd", ["f16", "bf16"])
def test_sixteen_bit_queries(main70, qd):
    case, q, idx, _ = main70
    if qd == "f16":
        q16 = q.astype(np.float16)
        wide, kw = q16.astype(np.float32), {}
    else:
        q16 = ref.round_bf16(q)
        wide, kw = ref.widen_bf16(q16), {"dtype": "bf16"}
    lists, counts = rq.select_lists_cpu(wide, case.c, EF, EPS)
    for raw in ("f32", "bf16"):
        rows = attach(idx, case.x, raw)
        got = rq.mstg_search(idx, q16, 10, EF, EPS, return_lists=True, refine_pool=40, exact=True, **kw)
        compare(got, case, wide, lists, counts, rows, 10, 40)
        dev = rq.mstg_search(idx, torch.from_numpy(q16.view(np.int16)).cuda().view(torch.float16 if qd == "f16" else torch.bfloat16), 10, EF, EPS,
                             return_lists=True, refine_pool=40, exact=True)
        torch.cuda.synchronize()
        assert all(bits_equal(a, b) for a, b in zip(got, dev))
    assert idx.query_dtype() == "f32"
    idx.set_rerank_vectors(case.x)


# ---- 8. borrowed 16-bit rows at 2 mod 4: the element path ------------------------------------------------------------------------
@pytest.mark.parametrize("raw", ["f16", "bf16"])
def test_borrowed_rows_at_2_mod_4_equal_the_aligned_attachment(raw):
    case, q = rref.main_case(7, 1)
    idx = case.device_index()
    x16 = case.x.astype(np.float16).view(np.uint16) if raw == "f16" else ref.round_bf16(case.x)
    attach(idx, case.x, raw)
    want = [rq.mstg_search(idx, q, 10, EF, EPS, refine_pool=p, exact=True) for p in (40, 4096)]
    flat = torch.from_numpy(x16.reshape(-1).view(np.int16).copy()).cuda()
    for first in (2, 1):  # the view starts at element 2 (4-byte aligned: the span path) | element 1 (2 mod 4: the element path)
        buf = torch.full((2 + flat.numel() + 2,), 0x7e00, dtype=torch.int16, device="cuda")  # (NaN guards around the rows)
        buf[first:first + flat.numel()] = flat
        torch.cuda.synchronize()
        ptr = buf.data_ptr() + 2 * first
        assert ptr % 4 == (0 if first == 2 else 2)
        idx.set_rerank_vectors(device_ptr=ptr, n=len(case.x), dtype=raw)
        got = [rq.mstg_search(idx, q, 10, EF, EPS, refine_pool=p, exact=True) for p in (40, 4096)]
        for w, g in zip(want, got):
            assert all(bits_equal(a, b) for a, b in zip(w, g)), first
        idx.set_rerank_vectors(None)
        del buf
    idx.close()


# ---- 9, 10, 11, 12. entries, chunks, variants, handles ------------------------------------------------------------------------------
def test_device_entry_on_a_side_stream_equals_the_host_entry(main70):
    case, q, idx, host = main70
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        tq = torch.from_numpy(q).cuda()
        dev = rq.mstg_search(idx, tq, 10, EF, EPS, return_lists=True, refine_pool=40, exact=True)
        short = rq.mstg_search(idx, tq, 10, EF, EPS, refine_pool=40, exact=True)
        zero = rq.mstg_search(idx, tq, 10, 0, EPS, refine_pool=40, exact=True)
    s.synchronize()
    assert all(bits_equal(a, b) for a, b in zip(host, dev))
    assert all(bits_equal(a, b) for a, b in zip(host[:3], short))
    assert not zero[2].cpu().numpy().any() and (zero[0].cpu().numpy() == -1).all()
    idx.release_stream(s.cuda_stream)


def test_result_does_not_depend_on_the_chunk_budget(main70):
    case, q, idx, want = main70
    tq = torch.from_numpy(q).cuda()
    try:
        for budget in (1, 60_000):
            idx.set_option("mstg_search_budget", budget)
            got = rq.mstg_search(idx, q, 10, EF, EPS, return_lists=True, refine_pool=40, exact=True)
            dev = rq.mstg_search(idx, tq, 10, EF, EPS, return_lists=True, refine_pool=40, exact=True)
            torch.cuda.synchronize()
            assert all(bits_equal(a, b) for a, b in zip(want, got)), budget
            assert all(bits_equal(a, b) for a, b in zip(want, dev)), budget
    finally:
        idx.set_option("mstg_search_budget", 0)


def test_numeric_variants_return_identical_bytes(main70):
    case, q, idx, want = main70
    try:
        for v in ("native_avx2", "portable", "native_avx512"):
            idx.set_numeric_variant(v)
            got = rq.mstg_search(idx, q, 10, EF, EPS, return_lists=True, refine_pool=40, exact=True)
            assert all(bits_equal(a, b) for a, b in zip(want, got)), v
    finally:
        idx.set_numeric_variant("native_avx512")


def test_other_handles_return_the_same_rows(main70):
    case, q, idx, want = main70
    cfg = dict(mf.DEFAULT_CONFIG, rabitq_bits=case.bits, faster_config=True, metric=case.metric, closure_epsilon=2.0)
    loaded, _ = mstg.load_mstg(mstg.save_mstg_bytes(idx, cfg))
    from_built = rq.IvfRabitqIndex.from_built(case.built_with_real_ids())
    for h in (loaded, from_built):
        h.set_rerank_vectors(case.x)
        got = rq.mstg_search(h, q, 10, EF, EPS, return_lists=True, refine_pool=40, exact=True)
        assert all(bits_equal(a, b) for a, b in zip(want, got))
        h.close()


# ---- 13. the binding -----------------------------------------------------------------------------------------------------------------
def test_binding():
    import closure_cases as cc
    x, _ = cc.clustered(600, 32, 8, 900)
    m = mstg.MstgIndex(32, "euclidean", max_posting_size=40, branching_factor=4, closure_epsilon=2.0, rabitq_bits=7, default_ef_search=6)
    m.fit(x)
    assert m.exact is False
    q = x[:20] + np.float32(0.01)
    refined_before = rq.mstg_search(m.handle, q, 10, 6, 0.6, refine_pool=100)
    m.set_rerank_vectors(x)
    m.set_query_arguments(refine_pool=100, exact=True)
    assert m.exact is True and m.refine_pool == 100 and m.default_ef_search == 6
    rows = m.batch_query(q, 10)
    ids, dist, cnt = rq.mstg_search(m.handle, q, 10, 6, 0.6, refine_pool=100, exact=True)
    for i, row in enumerate(rows):
        assert len(set(row[:, 0].tolist())) == len(row) == cnt[i] == 10
        assert np.array_equal(row[:, 1].view(np.uint32), dist[i, :cnt[i]].view(np.uint32))
        assert np.array_equal(row[:, 0], ids[i, :cnt[i]].astype(np.float32))
        assert np.array_equal(dist[i].view(np.uint32), ref.distances(q[i], x, ids[i], 0).view(np.uint32))  # exact, whatever the pool was
        assert (np.diff(dist[i]) >= 0).all()
    assert np.array_equal(m.query(q[0], 10), rows[0])
    # the option was put back after every call: a refined call on the same handle is the refined call of before
    assert all(bits_equal(a, b) for a, b in zip(refined_before, rq.mstg_search(m.handle, q, 10, 6, 0.6, refine_pool=100)))
    with pytest.raises(ValueError):
        rq.mstg_search(m.handle, q, 10, 6, 0.6, exact=True)
    m.set_query_arguments(ef_search=5)
    assert m.exact is True
    m.set_query_arguments(ef_search=6)
    # add swaps the handle: no vectors are attached to the new one, and nothing is re-attached silently
    extra = (x[:30] + np.float32(0.5)).astype(np.float32)
    first = m.add(extra)
    assert first == 600
    with pytest.raises(rq.RabitqError) as e:
        m.batch_query(q, 10)
    assert e.value.code == _abi.RBQ_INVALID_CONFIG and "raw vectors attached" in e.value.detail
    both = np.concatenate([x, extra])
    m.set_rerank_vectors(both)
    rows = m.batch_query(extra[:5], 10)
    for i, r in enumerate(rows):
        assert np.array_equal(r[:, 1].view(np.uint32), ref.distances(extra[i], both, r[:, 0].astype(np.uint64), 0).view(np.uint32))
    assert any((r[:, 0] >= 600).any() for r in rows)  # the new ids are served, by their own rows
    assert m.remove_ids(np.arange(600, 630, dtype=np.uint64)) > 0
    with pytest.raises(rq.RabitqError):
        m.batch_query(q, 10)
    m.set_query_arguments(exact=False)
    assert len(m.batch_query(q, 10)) == 20


# ---- 14. unchanged behaviour ----------------------------------------------------------------------------------------------------------
def raw_refined_call(idx, q, top_k, pool):
    """the C entry on prefilled outputs: (rc, ids, scores, counts)"""
    ids = np.full((len(q), top_k), 7, np.uint64)
    sc = np.full((len(q), top_k), 7.0, np.float32)
    cnt = np.full(len(q), 7, np.uint32)
    rc = lib().rbq_mstg_search_refined_batch(idx._h, _marshal.data_ptr(q), len(q), q.shape[1], top_k, EF, float(EPS), pool, ids.ctypes.data,
                                             sc.ctypes.data, cnt.ctypes.data, None, None)
    return rc, ids, sc, cnt


def test_option_off_and_other_entries_are_unchanged():
    case, q = rref.main_case(7, 0)
    idx = case.device_index()
    q = np.ascontiguousarray(q)
    refined = rq.mstg_search(idx, q, 10, EF, EPS, return_lists=True, refine_pool=40)
    plain = rq.mstg_search(idx, q, 10, EF, EPS, return_lists=True)
    # option on without vectors: refused, outputs untouched; settable all the same, and any non-zero value is 1
    idx.set_option("mstg_rerank", 5)
    v = C.c_int32(-1)
    assert lib().rbq_debug_copy_index(idx._h, b"mstg_rerank", C.byref(v), 4) == 0 and v.value == 1
    rc, ids, sc, cnt = raw_refined_call(idx, q, 10, 40)
    assert rc == _abi.RBQ_INVALID_CONFIG and (ids == 7).all() and (sc == 7.0).all() and (cnt == 7).all()
    with pytest.raises(rq.RabitqError) as e:
        rq.mstg_search(idx, q, 10, EF, EPS, refine_pool=40)
    assert e.value.code == _abi.RBQ_INVALID_CONFIG and "raw vectors attached" in e.value.detail
    with pytest.raises(rq.RabitqError):
        rq.mstg_search(idx, torch.from_numpy(q).cuda(), 10, EF, EPS, refine_pool=40)
    # the plain call ignores the option
    assert all(bits_equal(a, b) for a, b in zip(plain, rq.mstg_search(idx, q, 10, EF, EPS, return_lists=True)))
    # vectors attached, "rerank" 0: refused too
    idx.set_rerank_vectors(case.x)
    idx.set_option("rerank", 0)
    rc, ids, sc, cnt = raw_refined_call(idx, q, 10, 40)
    assert rc == _abi.RBQ_INVALID_CONFIG and (ids == 7).all() and (sc == 7.0).all() and (cnt == 7).all()
    with pytest.raises(rq.RabitqError) as e:
        rq.mstg_search(idx, q, 10, EF, EPS, refine_pool=40)
    assert "rerank 1" in e.value.detail
    idx.set_option("rerank", 1)
    exact = rq.mstg_search(idx, q, 10, EF, EPS, return_lists=True, refine_pool=40)  # (the option is on: this is the exact call)
    assert not bits_equal(exact[1], refined[1])
    assert all(bits_equal(a, b) for a, b in zip(plain, rq.mstg_search(idx, q, 10, EF, EPS, return_lists=True)))
    # option 0 with vectors attached: the refined call's bytes are those of the handle without vectors
    idx.set_option("mstg_rerank", 0)
    assert all(bits_equal(a, b) for a, b in zip(refined, rq.mstg_search(idx, q, 10, EF, EPS, return_lists=True, refine_pool=40)))
    assert all(bits_equal(a, b) for a, b in zip(exact, rq.mstg_search(idx, q, 10, EF, EPS, return_lists=True, refine_pool=40, exact=True)))
    assert lib().rbq_debug_copy_index(idx._h, b"mstg_rerank", C.byref(v), 4) == 0 and v.value == 0  # (put back after the call)
    idx.close()


# ---- 15. call order --------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_calls_before():
    case, q = rref.main_case(7, 0)
    tq = torch.from_numpy(q).cuda()
    calls = {"exact": dict(refine_pool=40, exact=True), "refined": dict(refine_pool=40), "plain": {}}
    first = {}
    for name, kw in calls.items():  # each call made first on a fresh handle
        h = case.device_index()
        h.set_rerank_vectors(case.x)
        first[name] = [t.cpu() for t in rq.mstg_search(h, tq, 10, EF, EPS, return_lists=True, **kw)]
        torch.cuda.synchronize()
        h.close()
    h = case.device_index()
    h.set_rerank_vectors(case.x)
    s = torch.cuda.Stream()
    got = []
    with torch.cuda.stream(s):
        tq2 = torch.from_numpy(q).cuda()
        for name in ("exact", "refined", "plain", "exact", "plain", "refined", "exact", "exact"):
            got.append((name, rq.mstg_search(h, tq2, 10, EF, EPS, return_lists=True, **calls[name])))
    s.synchronize()
    for name, g in got:
        assert all(bits_equal(a, b) for a, b in zip(first[name], g)), name
    h.release_stream(s.cuda_stream)
    h.close()


# ---- 16. recall, for the record ------------------------------------------------------------------------------------------------------
def test_recall_exact_is_not_below_refined():
    """7 bits, L2, pool 100: recall@10 against the truth by the same canonical distances (figures: DESIGN.md section 35)"""
    case, q = rref.recall_case()
    idx = case.device_index()
    idx.set_rerank_vectors(case.x)
    n = len(case.x)
    truth = np.stack([np.argsort(ref.distances(q[i], case.x, np.arange(n), 0), kind="stable")[:10] for i in range(len(q))]).astype(np.uint64)
    ri, _, rc = rq.mstg_search(idx, q, 10, 16, 0.6, refine_pool=100)
    ids, sc, cnt = run(idx, case, q, case.x, 10, 16, 0.6, 100)
    refined, exact = rref.recall_at(ri, rc, truth), rref.recall_at(ids, cnt, truth)
    print(f"recall@10, pool 100: refined {refined:.4f} exact {exact:.4f}")
    assert exact >= refined
    idx.close()
