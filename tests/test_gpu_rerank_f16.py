"""Raw vectors for the rerank kept as f16 or bf16 (option "rerank_raw_dtype").  The whole contract
is one equality: a search over 16-bit rows X16 returns, bit for bit, what the same search returns with widen(X16) attached as f32
on a handle that never heard of a dtype — ids, counts and score bits, through k_rerank and k_rerank_pool, on every entry.  Held
here against a second handle of the same index and against the NumPy restatement (tests/rerank_pool_ref.py) over widen(X16)."""
import functools

import numpy as np
import pytest

import rabitq_rs_amd as rq
from conftest import build_index, make_dataset
from rabitq_rs_amd import _abi
from rabitq_rs_amd import index as rq_index
from rerank_f16_ref import BF16, F16, round_to, widen
from rerank_pool_ref import NAN_BITS, PAD_ID, exact_scores, order_pool, rerank_pool

pytestmark = pytest.mark.gpu

N, NLIST, NQ = 3000, 12, 33  # (33 queries: some 8-lane groups and waves of the last pass have no candidate)
DTYPES = (F16, BF16)
QNAN = {F16: 0x7E00, BF16: 0x7FC0}


@functools.lru_cache(maxsize=None)
def _built(dim, metric, n=N, nlist=NLIST, bits=7, seed=2800):
    return build_index(n=n, dim=dim, nlist=nlist, total_bits=bits, metric=metric, normalize=(metric == 1 and dim > 1), seed=seed + dim)


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    _built.cache_clear()


def _queries(nq, dim, metric, seed=2890):
    return make_dataset(nq, dim, 3, seed + dim, normalize=(metric == 1 and dim > 1))


def _attach16(idx, x16, dtype, **kw):
    """host rows in 16 bits: f16 as a numpy.float16 array (dtype inferred), bf16 as its bit patterns"""
    if dtype == F16:
        idx.set_rerank_vectors(x16.view(np.float16), **kw)
    else:
        idx.set_rerank_vectors(x16, dtype="bf16", **kw)


def _attach_old(idx, rows):
    """f32 rows as before the option existed: the entry point alone, on a handle whose "rerank_raw_dtype" was never set"""
    rows = np.ascontiguousarray(rows, np.float32)
    assert rq_index.lib().rbq_index_set_rerank_vectors(idx._h, rows.ctypes.data, rows.shape[0]) == 0


class _Pair:
    """two handles of one built index: X16 attached as 16-bit rows, widen(X16) as f32 rows the old way"""

    def __init__(self, built, x16, dtype):
        self.x16, self.wide = x16, widen(x16, dtype)
        self.h16, self.h32 = rq.IvfRabitqIndex.from_built(built), rq.IvfRabitqIndex.from_built(built)
        _attach16(self.h16, x16, dtype)
        _attach_old(self.h32, self.wide)
        assert self.h16.rerank_dtype() == dtype and self.h32.rerank_dtype() == "f32"

    def close(self):
        self.h16.close()
        self.h32.close()


def _search(idx, q, top_k, nprobe, rerank, pool, **kw):
    idx.set_option("rerank", rerank)
    idx.set_rerank_pool(pool)
    try:
        ids, sc, cnt, _ = idx.batch_search_raw(q, rq.SearchParams(top_k, nprobe), **kw)
    finally:
        idx.set_rerank_pool(0)
        idx.set_option("rerank", 1)
    return ids, sc.view(np.uint32), cnt


def _assert_same(got, want, what=""):
    assert np.array_equal(got[2], want[2]), what
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what


def _restated(idx, wide, q, top_k, nprobe, pool, metric, nan_sign=None, **kw):
    """The restatement over `wide`: the pool is the plain search at top_k := pool (for the unpooled rerank: pool = top_k).
    nan_sign {(query, id): bits}: the bits a NaN score of the restatement is given before the entries are ordered
    (test_special_values says why); every other score, and which scores are NaN, stay the restatement's."""
    pid, _, pcnt = _search(idx, q, pool, nprobe, 0, 0, **kw)
    if nan_sign is None:
        return rerank_pool(q, wide, pid, pcnt, metric, top_k)
    ids, bits, counts = np.empty((len(q), top_k), np.uint64), np.empty((len(q), top_k), np.uint32), np.empty(len(q), np.uint32)
    for i in range(len(q)):
        c = int(pcnt[i])
        ex = exact_scores(q[i], wide, pid[i, :c], metric)
        for r in np.flatnonzero(np.isnan(ex) & (pid[i, :c] < wide.shape[0])):
            ex.view(np.uint32)[r] = nan_sign[(i, int(pid[i, r]))]
        ids[i], bits[i], counts[i] = order_pool(pid[i, :c], ex, c, metric, top_k)
    return ids, bits, counts


def _check_paths(pair, q, metric, paths, nprobe=8, nan_sign=None, **kw):
    for top_k, pool in paths:
        got = _search(pair.h16, q, top_k, nprobe, 1, pool, **kw)
        _assert_same(got, _search(pair.h32, q, top_k, nprobe, 1, pool, **kw), ("f32 handle", top_k, pool))
        _assert_same(got, _restated(pair.h32, pair.wide, q, top_k, nprobe, max(pool, top_k), metric, nan_sign=nan_sign, **kw),
                     ("restatement", top_k, pool))
        assert got[2].max() > 0


# ---- 1. same bits as f32 over the widened rows --------------------------------------------------------------------------------
PATHS = ((10, 0), (10, 32), (10, 200), (1100, 1500))  # k_rerank | k_rerank_pool below and above 1024 entries


@pytest.mark.parametrize("dim", [3, 8, 24, 56, 64, 72, 248, 256, 264, 520, 9, 65, 257])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_same_bits_as_f32_over_widened_rows(dtype, metric, dim):
    """3: tail only; 8, 24: a single / partial span (64 elements); 56, 64, 72: the span edge; 248, 256, 264: the step edge (4 spans);
    520: two steps and a chunk; 9, 65, 257: odd, the element path."""
    data, built = _built(dim, metric)
    pair = _Pair(built, round_to(data, dtype), dtype)
    try:
        _check_paths(pair, _queries(NQ, dim, metric), metric, PATHS)
    finally:
        pair.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_largest_lds_shape(dtype):
    """dim 2048 and pool 4096: the most dynamic LDS the kernel asks for; the pool ends at the index's 3000 vectors"""
    data, built = _built(2048, 0)
    pair = _Pair(built, round_to(data, dtype), dtype)
    try:
        _check_paths(pair, _queries(NQ, 2048, 0), 0, ((10, 4096),), nprobe=NLIST)
    finally:
        pair.close()


# ---- 2. special values ---------------------------------------------------------------------------------------------------------
def _special_rows(x16, dtype, dim, n_att):
    """Rows 0, n_att - 1 and a spread of others carry one special pattern each, in the main part or in the tail: one per row, so no
    sum meets +inf and -inf (an invalid operation's default NaN is the one value the CPU restatement may sign differently)."""
    main, tail = (1, 13 % (dim & ~7), (dim & ~7) - 1), tuple(range(dim & ~7, dim))
    if dtype == F16:
        vals = [0x0000, 0x8000, 0x0001, 0x8001, 0x0155, 0x03FF, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00]
    else:  # the same roles in bf16: zeros, smallest / mid / largest subnormal, largest finite, infinities, the quiet NaN
        vals = [0x0000, 0x8000, 0x0001, 0x8001, 0x0040, 0x007F, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0]
    rows = iter([0, n_att - 1] + list(range(5, n_att - 1, (n_att - 6) // (2 * len(vals)))))
    placed = []
    for i, v in enumerate(vals):
        for where in (main, tail):
            r = next(rows)
            x16[r, where[i % len(where)]] = v
            placed.append(r)
    x16[n_att - 1, dim - 1] = vals[8]  # +inf in the very last element of the attached array (beside the row's +0: no product of 0 and inf)
    return placed


@pytest.mark.parametrize("dim", [76, 77])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values(dtype, metric, dim):
    """zeros of both signs, subnormals, the largest finite values, infinities and the quiet NaN, in the main part and in the tail
    (dim 76: span path, 77: element path), rows 0 and n - 1 among them; 2500 of 3000 rows attached, so pooled ids past them score
    0x7fc00000.  Every vector is pooled and every score returned (pool 4096, top_k 3000).

    The equality with the f32 handle is over every bit, NaN rows included.  The restatement differs from the f32 kernels — the
    parent's, whose code this feature leaves as it is — in one bit: the sign of the NaN a row carrying a NaN scores under L2.
    Measured on an MI355X: q - NaN(0x7fc00000) gives 0xffc00000 in k_rerank and k_rerank_pool, for f32 rows as for 16-bit rows,
    where the oracle's x86 subtraction keeps 0x7fc00000 (IEEE 754 leaves the sign of a propagated NaN open; the products of the
    inner-product metric agree, 0x7fc00000 on both).  That sign decides whether those two rows are ordered first or last.  So for
    the rows that carry a NaN the restatement is given the sign the f32 handle returns; that such a row scores a NaN at all, every
    other score bit, the counts and the order rule remain the restatement's own."""
    data, built = _built(dim, metric)
    n_att = 2500
    x16 = round_to(data, dtype)[:n_att].copy()
    placed = _special_rows(x16, dtype, dim, n_att)
    assert 0 in placed and n_att - 1 in placed
    pair = _Pair(built, x16, dtype)
    try:
        q = _queries(NQ, dim, metric)
        f_ids, f_bits, _ = _search(pair.h32, q, 3000, NLIST, 1, 4096)
        carried = np.isnan(f_bits.view(np.float32)) & (f_ids < n_att)
        nan_sign = {(int(i), int(f_ids[i, r])): f_bits[i, r] for i, r in zip(*np.nonzero(carried))}
        assert set(id_ for _, id_ in nan_sign) == set(placed[-2:]) and len(nan_sign) == 2 * NQ
        assert all(int(b) & 0x7FFFFFFF == 0x7FC00000 for b in nan_sign.values())  # (the quiet NaN, whichever its sign)
        _check_paths(pair, q, metric, ((3000, 4096), (10, 200), (10, 0)), nprobe=NLIST, nan_sign=nan_sign)
        ids, bits, cnt = _search(pair.h16, q, 3000, NLIST, 1, 4096)
        assert (cnt == N).all()
        sc = bits.view(np.float32)
        assert (bits[ids >= n_att] == NAN_BITS).all() and (ids >= n_att).sum() == NQ * (N - n_att)
        assert np.isinf(sc).any() and (np.isnan(sc) & (ids < n_att)).sum() == 2 * NQ  # (the two rows that carry the quiet NaN)
    finally:
        pair.close()


# ---- 3. borrowed device rows, both alignments, guarded -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_borrowed_device_rows_both_alignments(dtype):
    import torch
    dim, metric = 64, 0
    data, built = _built(dim, metric)
    x16 = round_to(data, dtype)
    q = _queries(NQ, dim, metric)
    dev = torch.device("cuda", 0)
    flat = torch.from_numpy(x16.reshape(-1).view(np.int16).copy()).to(dev)
    guard = np.array([QNAN[dtype]], np.uint16).view(np.int16)[0]
    pair = _Pair(built, x16, dtype)
    other = rq.IvfRabitqIndex.from_built(built)
    try:
        for first in (2, 1):  # the view starts at element 2 (4-byte aligned: span path) | element 1 (2 mod 4: element path)
            buf = torch.full((2 + flat.numel() + 2,), int(guard), dtype=torch.int16, device=dev)
            buf[first:first + flat.numel()] = flat
            torch.cuda.synchronize(dev)
            ptr = buf.data_ptr() + 2 * first
            assert buf.data_ptr() % 16 == 0 and ptr % 4 == (0 if first == 2 else 2)
            other.set_rerank_vectors(device_ptr=ptr, n=N, dtype=dtype)
            assert other.rerank_dtype() == dtype
            for top_k, pool in PATHS:
                _assert_same(_search(other, q, top_k, 8, 1, pool), _search(pair.h16, q, top_k, 8, 1, pool), (first, top_k, pool))
            other.set_rerank_vectors(None)
            assert other.rerank_dtype() is None
            del buf
        with pytest.raises(rq.RabitqError, match="2-byte aligned"):
            other.set_rerank_vectors(device_ptr=flat.data_ptr() + 1, n=N - 1, dtype=dtype)
        assert other.rerank_dtype() is None
        # the same handle takes f32 rows again: the results of a handle that never saw 16-bit rows
        other.set_rerank_vectors(data)
        assert other.rerank_dtype() == "f32"
        plain = rq.IvfRabitqIndex.from_built(built)
        try:
            _attach_old(plain, data)
            for top_k, pool in PATHS:
                _assert_same(_search(other, q, top_k, 8, 1, pool), _search(plain, q, top_k, 8, 1, pool), ("f32 again", top_k, pool))
        finally:
            plain.close()
    finally:
        other.close()
        pair.close()


# ---- 4. filter and small counts ------------------------------------------------------------------------------------------------
def _filter_words(allowed, nbits):
    words = np.zeros((nbits + 31) // 32, np.uint32)
    allowed = np.asarray(allowed, np.int64)
    np.bitwise_or.at(words, allowed >> 5, (np.uint32(1) << (allowed & 31).astype(np.uint32)))
    return words


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_filter_and_small_counts(dtype, metric):
    dim = 72
    data, built = _built(dim, metric)
    pair = _Pair(built, round_to(data, dtype), dtype)
    early = rq.IvfRabitqIndex.from_built(built)
    try:
        q = _queries(NQ, dim, metric)
        few = dict(filter_words=_filter_words([3, 700, 701, 1500, 2999], N), filter_nbits=N)
        _check_paths(pair, q, metric, ((10, 200),), nprobe=NLIST, **few)
        got = _search(pair.h16, q, 10, NLIST, 1, 200, **few)
        assert (got[2] == 5).all() and (got[0][:, 5:] == PAD_ID).all() and (got[1][:, 5:] == NAN_BITS).all()
        # the pool option set before the rows are attached acts once they are
        early.set_rerank_pool(200)
        _attach16(early, pair.x16, dtype)
        ids, sc, cnt, _ = early.batch_search_raw(q, rq.SearchParams(10, 8))
        _assert_same((ids, sc.view(np.uint32), cnt), _search(pair.h16, q, 10, 8, 1, 200))
        unpooled = _search(pair.h16, q, 10, 8, 1, 0)
        assert not np.array_equal(ids, unpooled[0])  # (and it is the pool that acted)
    finally:
        early.close()
        pair.close()


# ---- 5. every entry agrees -----------------------------------------------------------------------------------------------------
def _every_entry(dtype, nq, devices):
    import torch
    dim, metric, top_k, nprobe, pool = 72, 0, 10, 8, 200
    data, built = _built(dim, metric)
    pair = _Pair(built, round_to(data, dtype), dtype)
    many = rq.IvfRabitqIndex.from_built(built, devices=devices)
    try:
        q = _queries(nq, dim, metric, seed=2900 + nq)
        for pl in (pool, 0):
            want = _search(pair.h32, q, top_k, nprobe, 1, pl)
            _assert_same(_search(pair.h16, q, top_k, nprobe, 1, pl), want, "host entry")
            pair.h16.set_rerank_pool(pl)
            try:
                out = pair.h16.batch_query(q, top_k, nprobe)
                assert len(out) == nq
                for i, o in enumerate(out):
                    c = int(want[2][i])
                    assert o.shape == (c, 2) and np.array_equal(o[:, 0], want[0][i, :c].astype(np.float32))
                    assert np.array_equal(o[:, 1].view(np.uint32), want[1][i, :c])
                dev = torch.device("cuda", 0)
                qd = torch.from_numpy(q).to(dev)
                d_i = torch.zeros(nq, top_k, dtype=torch.int64, device=dev)
                d_s = torch.zeros(nq, top_k, dtype=torch.float32, device=dev)
                d_c = torch.zeros(nq, dtype=torch.int32, device=dev)
                st = torch.cuda.Stream(dev)
                torch.cuda.synchronize(dev)
                pair.h16.search_batch_device(qd.data_ptr(), nq, dim, top_k, nprobe, d_i.data_ptr(), d_s.data_ptr(), d_c.data_ptr(),
                                             stream=st.cuda_stream)
                torch.cuda.synchronize(dev)
                pair.h16.release_stream(st.cuda_stream)
                _assert_same((d_i.cpu().numpy().view(np.uint64), d_s.cpu().numpy().view(np.uint32), d_c.cpu().numpy().view(np.uint32)), want,
                             "device entry")
            finally:
                pair.h16.set_rerank_pool(0)
        assert many.device_count() == 2
        _attach16(many, pair.x16, dtype)
        assert many.rerank_dtype() == dtype
        for pl in (pool, 0):
            _assert_same(_search(many, q, top_k, nprobe, 1, pl), _search(pair.h32, q, top_k, nprobe, 1, pl), "two replicas")
    finally:
        many.close()
        pair.close()


@pytest.mark.parametrize("nq", [1, NQ])
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_entry_agrees(dtype, nq):
    """the host entry, batch_query, the device entry on a caller's stream and two replicas on one device"""
    _every_entry(dtype, nq, [0, 0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_entry_agrees_on_two_devices(dtype):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    _every_entry(dtype, NQ, [0, 1])


# ---- 6. off means off ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_off_means_off(dtype):
    dim, metric = 72, 0
    data, built = _built(dim, metric)
    pair = _Pair(built, round_to(data, dtype), dtype)
    bare = rq.IvfRabitqIndex.from_built(built)
    try:
        q = _queries(NQ, dim, metric)
        assert bare.rerank_dtype() is None
        ref = bare.batch_search_raw(q, rq.SearchParams(10, 8))
        for pool in (0, 200):
            _assert_same(_search(pair.h16, q, 10, 8, 0, pool), (ref[0], ref[1].view(np.uint32), ref[2]), pool)
        want = _search(pair.h16, q, 10, 8, 1, 200)
        for bad in (3, -1):  # an unknown dtype is refused and the handle keeps what it had
            with pytest.raises(rq.RabitqError, match="dtype") as e:
                pair.h16.set_rerank_vectors(pair.wide, dtype=bad)
            assert e.value.code == _abi.RBQ_INVALID_CONFIG
            with pytest.raises(rq.RabitqError, match="dtype"):
                bare.set_rerank_vectors(pair.wide, dtype=bad)
            assert pair.h16.rerank_dtype() == dtype and bare.rerank_dtype() is None
            _assert_same(_search(pair.h16, q, 10, 8, 1, 200), want, bad)
        with pytest.raises(rq.RabitqError, match="unknown rerank dtype"):
            pair.h16.set_rerank_vectors(pair.wide, dtype="f64")
        # "f16" over an f32 host array rounds with astype(float16): the rows X16 holds already
        bare.set_rerank_vectors(data, dtype="f16")
        if dtype == F16:
            _assert_same(_search(bare, q, 10, 8, 1, 200), want, "astype")
        assert bare.rerank_dtype() == "f16"
    finally:
        bare.close()
        pair.close()


# ---- 7. recall -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_recall_rises_on_a_one_bit_index(dtype):
    """1-bit codes, rows rounded to 16 bits, pool 200: recall@10 against the float64 exact top 10 of the UNROUNDED rows is strictly
    above the unpooled recall (which is the plain search's: the unpooled rerank reorders the same ids)."""
    n, dim, nq, top_k, nprobe = 6000, 96, 200, 10, 8
    data, built = _built(dim, 0, n=n, nlist=16, bits=1, seed=2720)
    q = _queries(nq, dim, 0, seed=2830)
    d64 = ((q.astype(np.float64)[:, None, :] - data.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    truth = np.argsort(d64, axis=1, kind="stable")[:, :top_k]

    def recall(ids):
        return sum(len(set(ids[i].tolist()) & set(truth[i].tolist())) for i in range(nq)) / (nq * top_k)

    idx = rq.IvfRabitqIndex.from_built(built)
    try:
        _attach16(idx, round_to(data, dtype), dtype)
        unpooled = recall(_search(idx, q, top_k, nprobe, 1, 0)[0])
        pooled = recall(_search(idx, q, top_k, nprobe, 1, 200)[0])
        print(f"recall@10 {dtype}: unpooled {unpooled:.4f}, pool 200 {pooled:.4f}")
        assert pooled > unpooled, (unpooled, pooled)
    finally:
        idx.close()
