"""rbq_mstg_append / rbq_mstg_remove_ids (include/rbq_mstg_mutate.h): rows appended to and ids removed from a
device-resident MSTG index on the GPU.  The yardstick is never the new code: a mutated handle must equal, array for array and
byte for byte, the index the existing one-shot builder (rbq_mstg_build_device, itself pinned to the CPU builder by
tests/test_gpu_mstg_build.py) builds over the rows the index then holds, with the same centroids; its `.mstg` bytes and its
searches must equal that index's; the closure lists it reports must equal closure_assign_cpu's.  Every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import closure_cases as cc
import mstg_file as mf
import rabitq_rs_amd as rq
from rabitq_rs_amd import _abi, index, mstg

pytestmark = pytest.mark.gpu

ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
EPS, M, K = 2.0, 8, 24
N_ALL, N_OLD = 2200, 1500
# clustered(2200, dim, 24, seed): seeds at which the conditions test 1 asserts hold (found by a search over closure_assign_cpu)
SEEDS = {16: 9601, 64: 37973, 128: 25528, 208: 25528}


def _cfg(dim, bits, metric, faster):
    return rq.MstgIndex(dim, "euclidean" if metric == 0 else "angular", closure_epsilon=EPS, max_replicas=M, rabitq_bits=bits,
                        faster_config=faster).config()


def _build(x, c, bits, metric, faster, **kw):
    return rq.build_postings_on_device(x, c, bits, metric, closure_epsilon=EPS, max_replicas=M, faster_config=faster, **kw)


def _arrays(idx, bits):
    """the arrays tests/test_gpu_mstg_build.py compares, plus rnorm, bsumx and lsum"""
    D, ex, nlist = int(idx.dim), bits - 1, int(idx.cluster_count())
    Dc = (D + 63) // 64 * 64
    ln = idx.debug_copy_index("list_n", np.empty(nlist, np.uint32))
    nb = int(((ln.astype(np.int64) + 31) // 32).sum())
    cpu_u = 128 // ex if ex else 1
    w4 = ((D // 16 + cpu_u - 1) // cpu_u) if ex else 0
    sizes = {"list_gb0": nlist * 4, "list_n": nlist * 4, "centroids": nlist * D * 4, "blocks": nb * (Dc * 4 + 384), "ids": nb * 256,
             "bsum": nb * 32, "lsum": nlist * 32, "bsumx": nb * 32, "delta": nb * 128, "vl": nb * 128, "rnorm": nb * 128,
             "cent_hi": nlist * D * 2, "cent_lo": nlist * D * 2, "cnorm2": nlist * 4}
    if ex:
        sizes.update({"ex": nb * 32 * w4 * 256, "fadd_ex": nb * 128, "fres_ex": nb * 128})
    return {name: idx.debug_copy_index(name, np.empty(nbytes, np.uint8)) for name, nbytes in sizes.items()}


def _same(ref, got, bits, cfg=None, idmap=None, what=""):
    """every array; with `idmap`, ref's real ids j stand for idmap[j]; without it the saved bytes are compared too"""
    a, b = _arrays(ref, bits), _arrays(got, bits)
    assert a.keys() == b.keys()
    for name in a:
        assert a[name].size == b[name].size, (what, name, a[name].size, b[name].size)
        want = a[name]
        if name == "ids" and idmap is not None:
            j = want.view(np.uint64)
            want = np.where(j == ONES, ONES, np.asarray(idmap, np.uint64)[np.where(j == ONES, 0, j).astype(np.int64)]).view(np.uint8)
        bad = np.nonzero(want != b[name])[0]
        assert bad.size == 0, f"{what} {name}: {bad.size} bytes differ, first at {bad[:5]}"
    assert len(ref) == len(got) and ref.cluster_count() == got.cluster_count()
    if cfg is not None and idmap is None:
        assert mstg.save_mstg_bytes(got, cfg) == mstg.save_mstg_bytes(ref, cfg), what


def _queries(x, nq=48, seed=5):
    rng = np.random.default_rng(seed)
    return (x[rng.integers(0, len(x), nq)] + 0.01 * rng.standard_normal((nq, x.shape[1]))).astype(np.float32)


def _answers(h, q, idmap=None):
    """mstg_search and the refined search (refine_pool 64): ids (mapped), counts, score bits"""
    out = []
    for pool in (None, 64):
        ids, sc, cnt = mstg.mstg_search(h, q, 10, 6, 0.6, refine_pool=pool)
        ids = ids.copy()
        for i in range(len(q)):
            ids[i, cnt[i]:] = 0
            if idmap is not None:
                ids[i, :cnt[i]] = np.asarray(idmap, np.uint64)[ids[i, :cnt[i]].astype(np.int64)]
        sc = sc.copy().view(np.uint32)
        for i in range(len(q)):
            sc[i, cnt[i]:] = 0
        out += [ids, cnt.copy(), sc]
    return out


def _same_answers(a, b):
    assert int(a[1].sum()) > 0
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def _pairs_per_list(lists, counts, k):
    keep = np.arange(lists.shape[1])[None, :] < counts[:, None]
    return np.bincount(lists[keep].astype(np.int64), minlength=k)


@functools.lru_cache(maxsize=None)
def _data(dim):
    x, c = cc.clustered(N_ALL, dim, K, SEEDS[dim])
    lists, counts = rq.closure_assign_cpu(x, c, EPS, M)
    return x, c, lists, counts  # shared by the tests: computed once, never written


# ---- 1. append equals the one-shot build ---------------------------------------------------------------------------------------
CASES = [pytest.param(64, b, m, f, id=f"d64_{b}bit_{'ip' if m else 'l2'}_{'const' if f else 'optimal'}")
         for b in (1, 3, 7) for m in (0, 1) for f in (True, False)]
CASES += [pytest.param(d, 7, 0, True, id=f"d{d}_7bit_l2_const") for d in (16, 128, 208)]  # Dc 64, 128, 256: the 8-byte tail granule


@pytest.mark.parametrize("dim,bits,metric,faster", CASES)
def test_append_equals_the_one_shot_build(dim, bits, metric, faster):
    x, c, lists, counts = _data(dim)
    old_n, new_n = _pairs_per_list(lists[:N_OLD], counts[:N_OLD], K), _pairs_per_list(lists[N_OLD:], counts[N_OLD:], K)
    assert old_n.sum() >= 1.1 * N_OLD and new_n.sum() >= 1.1 * (N_ALL - N_OLD)
    assert (old_n % 32 != 0).any(), "no list has a partly filled tail block before the append"
    assert (new_n == 0).any(), "every list receives something"
    cfg = _cfg(dim, bits, metric, faster)
    old, ref = _build(x[:N_OLD], c, bits, metric, faster), _build(x, c, bits, metric, faster)
    assert old.id_bound() == N_OLD
    got, gl, gc = mstg.append_postings(old, x[N_OLD:], closure_epsilon=EPS, max_replicas=M, return_lists=True)
    assert np.array_equal(gc, counts[N_OLD:]) and np.array_equal(gl, lists[N_OLD:])
    _same(ref, got, bits, cfg, what="append")
    assert got.id_bound() == N_ALL and len(got) == int(counts.sum())
    for h in (old, ref, got):
        h.close()


# ---- 2. a list that is empty before the append ------------------------------------------------------------------------------------
def test_append_into_a_list_that_was_empty():
    x, c, _, _ = _data(64)
    rng = np.random.default_rng(71)
    far = np.zeros((2, 64), np.float32)
    far[0, 0], far[1, 1] = 60.0, -80.0
    c2 = np.concatenate([c, far]).astype(np.float32)
    near = (far[0] + 0.05 * rng.standard_normal((60, 64))).astype(np.float32)
    new = np.concatenate([x[N_OLD:N_OLD + 100], near]).astype(np.float32)
    full = np.concatenate([x[:N_OLD], new]).astype(np.float32)
    cfg = _cfg(64, 7, 0, True)
    old, ref = _build(x[:N_OLD], c2, 7, 0, True), _build(full, c2, 7, 0, True)
    ln_old = old.debug_copy_index("list_n", np.empty(K + 2, np.uint32))
    assert ln_old[K] == 0 and ln_old[K + 1] == 0
    got = mstg.append_postings(old, torch.from_numpy(new).cuda(), closure_epsilon=EPS, max_replicas=M)
    ln = got.debug_copy_index("list_n", np.empty(K + 2, np.uint32))
    assert ln[K] == 60 and ln[K + 1] == 0
    _same(ref, got, 7, cfg, what="empty list")
    _, parsed, _, _, _ = mf.parse(mstg.save_mstg_bytes(got, cfg))
    assert len(parsed[K]["ids"]) == 60 and len(parsed[K + 1]["ids"]) == 0
    for h in (old, ref, got):
        h.close()


# ---- 3. three appends, chunked, host and device input ---------------------------------------------------------------------------
def test_three_chunked_appends_from_host_and_device_memory():
    """a base of 100 rows, then 600 + 900 + 700"""
    x, c = cc.clustered(2300, 64, K, 913)
    cuts = [100, 700, 1600, 2300]
    cfg = _cfg(64, 7, 0, False)
    ref = _build(x, c, 7, 0, False)
    results = []
    for chunk in (64, 0):
        before = mstg.append_passes()
        h = _build(x[:100], c, 7, 0, False)
        for j in range(3):
            part = x[cuts[j]:cuts[j + 1]]
            data = torch.from_numpy(part).cuda() if j == 1 else part
            nxt = mstg.append_postings(h, data, closure_epsilon=EPS, max_replicas=M, max_chunk_rows=chunk)
            h.close()
            h = nxt
        passes = mstg.append_passes() - before
        print("max_chunk_rows", chunk, "encode passes", passes)
        assert passes > 3 if chunk else passes == 3
        _same(ref, h, 7, cfg, what=f"chunk {chunk}")
        results.append(h)
    a, b = _arrays(results[0], 7), _arrays(results[1], 7)
    assert all(np.array_equal(a[n], b[n]) for n in a)
    for h in results + [ref]:
        h.close()


# ---- 4. the shortlist path ----------------------------------------------------------------------------------------------------
def test_append_through_the_gemm_shortlist():
    x, c = cc.clustered(500, 32, 300, 41)  # more than RBQ_MSTG_SHORTLIST lists
    lists, counts = rq.closure_assign_cpu(x, c, EPS, M)
    cfg = _cfg(32, 7, 0, True)
    old, ref = _build(x[:400], c, 7, 0, True), _build(x, c, 7, 0, True)
    before = mstg.closure_fallbacks()
    got, gl, gc = mstg.append_postings(old, x[400:], closure_epsilon=EPS, max_replicas=M, return_lists=True)
    print("closure fallbacks before", before, "after", mstg.closure_fallbacks(), "of 100 rows")
    assert np.array_equal(gc, counts[400:]) and np.array_equal(gl, lists[400:])
    _same(ref, got, 7, cfg, what="shortlist")
    for h in (old, ref, got):
        h.close()


# ---- 5. a loaded handle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("faster", [True, False])
def test_append_to_a_loaded_handle(faster):
    x, c, _, counts = _data(64)
    cfg = _cfg(64, 7, 0, faster)
    old, ref = _build(x[:N_OLD], c, 7, 0, faster), _build(x, c, 7, 0, faster)
    back, _ = mstg.load_mstg(mstg.save_mstg_bytes(old, cfg))
    got, gl, gc = mstg.append_postings(back, torch.from_numpy(x[N_OLD:]).cuda(), closure_epsilon=EPS, max_replicas=M, return_lists=True)
    assert np.array_equal(gc.cpu().numpy().view(np.uint32), counts[N_OLD:])
    assert mstg.save_mstg_bytes(got, cfg) == mstg.save_mstg_bytes(ref, cfg)
    q = _queries(x)
    _same_answers(_answers(ref, q), _answers(got, q))
    for h in (old, ref, back, got):
        h.close()


# ---- 6. remove equals the build over the kept rows ------------------------------------------------------------------------------
def _kept(n, gone):
    keep = np.ones(n, bool)
    g = np.asarray(gone, np.uint64)
    keep[g[g < n].astype(np.int64)] = False
    return np.nonzero(keep)[0]


@pytest.mark.parametrize("metric", [0, 1])
def test_remove_equals_the_build_over_the_kept_rows(metric):
    x, c, lists, counts = _data(64)
    rng = np.random.default_rng(83 + metric)
    gone = rng.choice(N_ALL, N_ALL // 10, replace=False).astype(np.uint64)
    ids = np.concatenate([gone, gone[:40], np.array([N_ALL, N_ALL + 7, 2 ** 63 + 5, 2 ** 64 - 1], np.uint64)])
    rng.shuffle(ids)
    Kr = _kept(N_ALL, gone)
    full, ref = _build(x, c, 7, metric, True), _build(x[Kr], c, 7, metric, True)
    want_removed = int(counts[gone.astype(np.int64)].sum())
    for src in (ids, torch.from_numpy(ids.view(np.int64)).cuda()):
        got, removed = mstg.remove_postings(full, src)
        assert removed == want_removed
        _same(ref, got, 7, idmap=Kr, what="remove")
        assert got.id_bound() == int(Kr.max()) + 1
        got.close()
    full.close()
    ref.close()


def test_remove_every_member_of_a_list():
    x, c, lists, counts = _data(64)
    keep = np.arange(M)[None, :] < counts[:, None]
    target = int(np.argmin(_pairs_per_list(lists, counts, K)))
    gone = np.nonzero(((lists == target) & keep).any(axis=1))[0].astype(np.uint64)
    assert 0 < len(gone) < N_ALL
    Kr = _kept(N_ALL, gone)
    cfg = _cfg(64, 7, 0, True)
    full, ref = _build(x, c, 7, 0, True), _build(x[Kr], c, 7, 0, True)
    got, removed = mstg.remove_postings(full, gone)
    assert removed == int(counts[gone.astype(np.int64)].sum())
    assert got.debug_copy_index("list_n", np.empty(K, np.uint32))[target] == 0
    _same(ref, got, 7, idmap=Kr, what="emptied list")
    ca, la, ia, _, _ = mf.parse(mstg.save_mstg_bytes(ref, cfg))
    cb, lb, ib, _, _ = mf.parse(mstg.save_mstg_bytes(got, cfg))
    assert ca == cb and np.array_equal(ia, ib) and len(la) == len(lb) == K
    assert len(lb[target]["ids"]) == 0
    for A, B in zip(la, lb):
        assert A.keys() == B.keys()
        for f in A:
            if f in ("off", "rec0"):
                assert A[f] == B[f]
            elif f == "config":
                assert A[f][0] == B[f][0] and (A[f][1] is None) == (B[f][1] is None)
                assert A[f][1] is None or np.float32(A[f][1]).view(np.uint32) == np.float32(B[f][1]).view(np.uint32)
            elif f == "ids":
                assert np.array_equal(Kr[A[f].astype(np.int64)].astype(np.uint64), B[f])
            elif f == "cluster_id":
                assert A[f] == B[f]
            else:
                assert np.array_equal(np.ascontiguousarray(A[f]).view(np.uint8), np.ascontiguousarray(B[f]).view(np.uint8)), f
    for h in (full, ref, got):
        h.close()


# ---- 7. a sequence ------------------------------------------------------------------------------------------------------------
def test_a_sequence_of_removes_and_adds_with_a_save_and_a_load():
    x, c, _, _ = _data(64)
    cfg = _cfg(64, 7, 0, True)
    rng = np.random.default_rng(97)
    live = {i: x[i] for i in range(1000)}  # id -> row: the model
    h = _build(x[:1000], c, 7, 0, True)

    def remove(ids):
        nonlocal h
        nxt, _ = mstg.remove_postings(h, np.asarray(ids, np.uint64))
        h.close()
        h = nxt
        for i in ids:
            live.pop(int(i), None)

    def add(rows):
        nonlocal h
        first = max(live) + 1
        assert h.id_bound() == first
        nxt = mstg.append_postings(h, rows, closure_epsilon=EPS, max_replicas=M, max_chunk_rows=150)
        h.close()
        h = nxt
        for j, r in enumerate(rows):
            live[first + j] = r

    remove(rng.choice(1000, 120, replace=False))
    add(x[1000:1500])
    remove(list(rng.choice(1500, 200, replace=False)) + [1499, 1498])  # (the top ids go: the bound shrinks)
    back, _ = mstg.load_mstg(mstg.save_mstg_bytes(h, cfg))
    h.close()
    h = back
    add(x[1500:2100])
    order = np.array(sorted(live), np.int64)
    rows = np.stack([live[int(i)] for i in order]).astype(np.float32)
    ref = _build(rows, c, 7, 0, True)
    _same(ref, h, 7, idmap=order, what="sequence")
    ca, la, _, _, _ = mf.parse(mstg.save_mstg_bytes(ref, cfg))
    cb, lb, _, _, _ = mf.parse(mstg.save_mstg_bytes(h, cfg))
    assert ca == cb
    for A, B in zip(la, lb):
        assert np.array_equal(order[A["ids"].astype(np.int64)].astype(np.uint64), B["ids"])
        for f in ("code", "bits", "ex") + tuple(mf.FACTORS):
            assert np.array_equal(np.ascontiguousarray(A[f]).view(np.uint8), np.ascontiguousarray(B[f]).view(np.uint8)), f
    q = _queries(rows)
    _same_answers(_answers(ref, q, idmap=order), _answers(h, q))
    ref.close()
    h.close()


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------
def _raw_append(h, x, first_id, eps=EPS, m=M):
    out = C.c_void_p(0xDEAD)
    rc = index.lib().rbq_mstg_append(h._h if h is not None else None, x.ctypes.data if x is not None else None,
                                     0 if x is None else len(x), first_id, eps, m, 0, None, None, C.byref(out))
    return rc, index._detail(), out.value


def _raw_remove(h, ids, n=None):
    out, removed = C.c_void_p(0xDEAD), C.c_uint64(77)
    rc = index.lib().rbq_mstg_remove_ids(h._h if h is not None else None, ids.ctypes.data if ids is not None else None,
                                         (len(ids) if ids is not None else 3) if n is None else n, C.byref(removed), C.byref(out))
    return rc, index._detail(), out.value


def test_errors_leave_the_handle_untouched():
    x, c, _, _ = _data(64)
    h = _build(x[:N_OLD], c, 7, 0, True)
    q = _queries(x)
    before = _answers(h, q)
    new = np.ascontiguousarray(x[N_OLD:N_OLD + 50])
    bad = new.copy()
    bad[17, 3] = np.inf
    INV = _abi.RBQ_INVALID_CONFIG
    # an IVF handle, and a posting-list handle made by rbq_index_create_with_recon (no residual norms)
    built = rq.builder.train(x[:600], 8, 7, rq.Metric.L2, rq.RotatorType.FhtKacRotator, 42, True, kmeans_iters=2)
    ivf = rq.IvfRabitqIndex.from_built(built)
    pl_built = rq.builder.train_with_clusters(x[:300], c, np.zeros(300, np.uint32), 7, 0, rq.RotatorType.NoRotation, 42, True)
    created = rq.IvfRabitqIndex.from_built(pl_built)
    ids = np.arange(5, dtype=np.uint64)
    cases = [
        (_raw_append(ivf, new, 10 ** 6), "not a posting-list handle: use rbq_index_append"),
        (_raw_remove(ivf, ids), "not a posting-list handle: use rbq_index_remove_ids"),
        (_raw_append(created, new, 10 ** 6), "the handle holds no residual norms or reconstruction factors (rbq_index_create*): "
                                             "the grown index could not be saved"),
        (_raw_remove(created, ids), "the handle holds no residual norms or reconstruction factors (rbq_index_create*): "
                                    "the shrunk index could not be saved"),
        (_raw_append(h, new, N_OLD - 1), f"first_id {N_OLD - 1} is below the index's id bound {N_OLD}"),
        (_raw_append(h, new[:0], N_OLD), "no vectors"),
        (_raw_append(h, None, N_OLD), "null vectors"),
        (_raw_append(h, new, N_OLD, m=0), "max_replicas must be positive"),
        (_raw_append(h, new, N_OLD, m=65), "max_replicas above 64 is not supported"),
        (_raw_append(h, new, N_OLD, eps=-0.5), "closure epsilon must be finite and not negative"),
        (_raw_append(h, new, N_OLD, eps=float("nan")), "closure epsilon must be finite and not negative"),
        (_raw_append(h, bad, N_OLD), "closure assignment input must be finite"),
        (_raw_append(h, new, 2 ** 64 - 20), "the new ids pass 2^64 - 1"),
        (_raw_remove(h, None), "null ids"),
        (_raw_remove(h, ids, n=0), "no ids"),
        (_raw_remove(h, np.arange(N_OLD, dtype=np.uint64)),
         "the ids cover every vector of the index: an index without vectors cannot be built"),
        (_raw_append(None, new, 0), "null index"),
        (_raw_remove(None, ids), "null index"),
    ]
    for (rc, detail, out), want in cases:
        assert rc == INV and detail == want and not out, (rc, detail, out, want)
    # the IVF entry points keep refusing posting-list handles with their messages
    L = index.lib()
    out = C.c_void_p(0xDEAD)
    rc = L.rbq_index_append(h._h, new.ctypes.data, None, len(new), N_OLD, 0, 1.0, 0, 1, None, None, C.byref(out))
    assert rc == INV and index._detail() == "posting-list handles (RBQ_ROTATOR_NONE) cannot be appended to" and not out.value
    out = C.c_void_p(0xDEAD)
    rc = L.rbq_index_remove_ids(h._h, ids.ctypes.data, len(ids), 1, None, None, C.byref(out))
    assert rc == INV and index._detail() == "posting-list handles (RBQ_ROTATOR_NONE) cannot be removed from" and not out.value
    _same_answers(before, _answers(h, q))
    assert h.id_bound() == N_OLD
    for o in (h, ivf, created):
        o.close()
    built.close()
    pl_built.close()


# ---- 9. Python ------------------------------------------------------------------------------------------------------------------
def test_mstg_index_add_and_remove_ids(tmp_path):
    x, _, _, _ = _data(64)
    a, b, cpart = x[:1200], x[1200:1800], x[1800:]
    ix = rq.MstgIndex(64, max_posting_size=64, closure_epsilon=0.5, max_replicas=4).fit(a)
    assert len(ix) == ix.id_bound() == 1200
    assert ix.add(b) == 1200
    assert ix.add(torch.from_numpy(cpart).cuda()) == 1800
    assert len(ix) == ix.id_bound() == N_ALL
    ref = rq.MstgIndex(64, max_posting_size=64, closure_epsilon=0.5, max_replicas=4)
    ref.handle = rq.build_postings_on_device(x, ix.centroids, 7, 0, closure_epsilon=0.5, max_replicas=4, faster_config=True)
    ref.centroids, ref._n = ix.centroids, N_ALL
    q = _queries(x, 32)
    for r1, r2 in zip(ix.batch_query(q, 10), ref.batch_query(q, 10)):
        assert r1.shape[0] > 0 and np.array_equal(r1.view(np.uint32), r2.view(np.uint32))
    removed = ix.remove_ids(np.arange(2100, N_ALL, dtype=np.uint64))
    assert removed >= 100 and len(ix) == ix.id_bound() == 2100
    want = ix.batch_query(q, 10)
    ix.save(tmp_path / "m")
    back = rq.MstgIndex.load(tmp_path / "m")
    assert len(back) == 2100 and back.id_bound() == 2100
    for r1, r2 in zip(want, back.batch_query(q, 10)):
        assert np.array_equal(r1.view(np.uint32), r2.view(np.uint32))
    for bad in (np.zeros((3, 32), np.float32), np.zeros(64, np.float32)):
        with pytest.raises(ValueError):
            ix.add(bad)
    with pytest.raises(RuntimeError):
        rq.MstgIndex(64).add(a)
    with pytest.raises(RuntimeError):
        rq.MstgIndex(64).remove_ids([1])
