"""CPU side of the ranking GEMM's error budget (tests/rank_bound.py): the numpy restatements are pinned to
hand-written bit patterns and to the oracle, and the checker that test_gpu_rank_bound.py applies to the GPU's score
rows rejects every row a broken GEMM would write."""
import ctypes as C

import numpy as np
import pytest

import oracle
import rabitq_rs_amd as rq
import rank_bound as rb
from conftest import make_dataset


def _bits(u):
    return np.array(u, dtype=np.uint32).view(np.float32)


# (x bits, hi bits, lo bits)
SPLIT_KAT = [
    (0x3F800000, 0x3F80, 0x0000),  # 1.0: exact
    (0x3F808000, 0x3F80, 0x3B80),  # 1 + 2^-8: a tie, rounds DOWN to the even 0x3F80; lo = 2^-8
    (0x3F818000, 0x3F82, 0xBB80),  # 1 + 2^-7 + 2^-8: a tie, rounds UP to the even 0x3F82; lo = -2^-8
    (0x3F808001, 0x3F81, 0xBB80),  # just above the tie: up; lo = bf16(-2^-8 + 2^-23) = -2^-8
    (0x3F7FFF80, 0x3F80, 0xB700),  # 1 - 2^-17: the carry crosses into the next binade (1.0); lo = -2^-17
    (0xBF7FFF80, 0xBF80, 0x3700),  # and its negative
    (0x80000000, 0x8000, 0x0000),  # -0.0: hi keeps the sign; lo = -0 - (-0) = +0
    (0x00000000, 0x0000, 0x0000),
    (0x00000001, 0x0000, 0x0000),  # smallest f32 subnormal: hi and lo round to +0
    (0x00008000, 0x0000, 0x0000),  # 2^-134, half of bf16's smallest subnormal: a tie, to the even 0
    (0x00018000, 0x0002, 0x8000),  # 1.5 bf16 subnormal units: a tie, up to 2; lo = -2^-134, a tie to -0
    (0x00010001, 0x0001, 0x0000),  # 2^-133 + 2^-149: hi = 2^-133, lo rounds the 2^-149 away
    (0x007FFFFF, 0x0080, 0x8000),  # largest subnormal: carries into the smallest normal; lo = -2^-149 -> -0
    (0x7F7F7FFF, 0x7F7F, 0x7B00),  # largest f32 whose hi stays finite; lo = 2^119 - 2^104 rounded = 2^119
    (0x7F7F8000, 0x7F80, 0xFF80),  # smallest f32 that rounds to inf (a tie, to the even 0x7F80); lo = x - inf = -inf
    (0x7F7FFFFF, 0x7F80, 0xFF80),  # FLT_MAX: inf
    (0xFF7F8000, 0xFF80, 0x7F80),  # negative: -inf, lo = +inf
    (0x7F800000, 0x7F80, 0xFFC0),  # inf: hi inf, lo = bf16(inf - inf) = the default NaN (sign set on x86), quiet
]


def test_bf16_split_known_answers():
    x = _bits([k[0] for k in SPLIT_KAT])
    hi, lo = rb.bf16_split(x)
    for i, (xb, h, lob) in enumerate(SPLIT_KAT):
        if xb == 0x7F800000:  # inf - inf: a NaN whose sign is the platform's; only its being a quiet NaN is pinned
            assert hi[i] == h and (int(lo[i]) & 0x7FC0) == 0x7FC0, f"{xb:#010x}: {hi[i]:#06x} {lo[i]:#06x}"
            continue
        assert (int(hi[i]), int(lo[i])) == (h, lob), f"x={xb:#010x}: hi={hi[i]:#06x} lo={lo[i]:#06x}, want {h:#06x} {lob:#06x}"


def test_bf16_rne_nan_stays_nan():
    x = _bits([0x7FC00000, 0x7F800001, 0xFFFFFFFF])
    h = rb.bf16_rne(x)
    assert ((h & 0x7F80) == 0x7F80).all() and ((h & 0x40) != 0).all()


def test_bf16_split_residual_bound():
    """|x - hi - lo| <= 2^-16 |x| over every binade of normal f32 and a sweep of mantissas; the absolute floor of
    subnormal lo (2^-134) is what the checker adds for tiny x, and it is tight there."""
    rng = np.random.default_rng(3)
    u = rng.integers(0x00800000, 0x7F7F0000, 200000, dtype=np.uint64).astype(np.uint32)
    u |= (rng.integers(0, 2, u.size, dtype=np.uint32) << 31)
    x = u.view(np.float32)
    hi, lo = rb.bf16_split(x)
    assert rb.split_residual_ok(x, hi, lo).all()
    big = np.abs(x) >= 2.0 ** -100  # lo is normal: the relative bound alone holds
    r = np.abs(x[big].astype(np.float64) - rb.bf16_to_f32(hi[big]) - rb.bf16_to_f32(lo[big]))
    assert (r <= rb.SPLIT_REL * np.abs(x[big].astype(np.float64))).all()
    # just above the smallest normal, x - hi is a bf16 subnormal: its rounding exceeds 2^-16 |x| and is covered by
    # the absolute floor alone
    tiny = _bits([0x00818001])
    h, lo_ = rb.bf16_split(tiny)
    r = abs(float(tiny[0]) - float(rb.bf16_to_f32(h)[0]) - float(rb.bf16_to_f32(lo_)[0]))
    assert r > rb.SPLIT_REL * float(tiny[0]) and rb.split_residual_ok(tiny, h, lo_).all()


def test_canonical_matches_oracle():
    """The numpy restatement of ref_l2_distance_sqr / ref_dot equals the oracle bit for bit, with and without a tail."""
    L = oracle.lib()
    f32p = C.POINTER(C.c_float)
    rng = np.random.default_rng(5)
    for D in (8, 13, 64, 100, 960):
        q = (rng.standard_normal((64, D)) * rng.choice([1e-3, 1.0, 1e3], (64, 1))).astype(np.float32)
        c = rng.standard_normal((64, D)).astype(np.float32)
        for metric in (0, 1):
            got = rb.canonical(q, c, metric)
            fn = L.ref_l2_distance_sqr if metric == 0 else L.ref_dot
            want = np.array([fn(q[i].ctypes.data_as(f32p), c[i].ctypes.data_as(f32p), D) for i in range(64)], np.float32)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (D, metric)


def test_select_eps_matches_formula():
    D, qn, cm = 960, np.float32(123.5), np.float32(77.25)
    want = ((6 * D + 16) * 2.0 ** -24 + 4 * 2.0 ** -16) * (float(qn) + float(cm)) * 1.001
    assert abs(float(rb.select_eps(D, qn, cm)) - want) <= 1e-6 * want


# ---- the checker has teeth ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def operands():
    """Real rotated queries and centroids of a small CPU-built index (FHT-Kac, D 256 = 8 slabs of 32)."""
    dim, nlist = 256, 130
    data = make_dataset(3000, dim, 32, 41)
    rng = np.random.default_rng(42)
    cent = data[rng.choice(len(data), nlist, replace=False)].copy()
    d2 = (data ** 2).sum(1)[:, None] + (cent ** 2).sum(1)[None, :] - 2 * data @ cent.T
    built = rq.builder.train_with_clusters(data, cent, d2.argmin(1).astype(np.uint32), 7, 0, 1, 43, True)
    q = make_dataset(70, dim, 32, 44)
    rot = np.stack([built.rotate(x) for x in q])
    rcent = np.stack([built.centroid(c) for c in range(nlist)])
    built.close()
    return rot, rcent


def _rows(rot, cent, metric, drop=None):
    """Score rows in float64 rounded to f32, the K range `drop` (a slice) left out of the dot product."""
    q = rot.astype(np.float64)
    c = cent.astype(np.float64)
    dot = q @ c.T
    if drop is not None:
        dot = dot - q[:, drop] @ c[:, drop].T
    if metric == 1:
        return dot.astype(np.float32)
    return ((q * q).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2 * dot).astype(np.float32)


def _split_gemm(rot, cent, metric):
    """What a correct split-bf16 GEMM computes: qh.ch + qh.cl + ql.ch exactly, rounded once."""
    qh, ql = (rb.bf16_to_f32(h).astype(np.float64) for h in rb.bf16_split(rot))
    ch, cl = (rb.bf16_to_f32(h).astype(np.float64) for h in rb.bf16_split(cent))
    dot = qh @ ch.T + qh @ cl.T + ql @ ch.T
    if metric == 1:
        return dot.astype(np.float32)
    q, c = rot.astype(np.float64), cent.astype(np.float64)
    return ((q * q).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2 * dot).astype(np.float32)


@pytest.mark.parametrize("metric", [0, 1])
def test_checker_accepts_correct_rows(operands, metric):
    rot, cent = operands
    D = rot.shape[1]
    for A in (_rows(rot, cent, metric), _split_gemm(rot, cent, metric)):
        worst, bad, _ = rb.check_rows(A, rot, cent, metric, D)
        assert not bad and worst <= 1.0, (worst, bad[:5])
    # the margin the split leaves: a split GEMM sits well inside the budget, so the faults below are not near it
    worst, _, _ = rb.check_rows(_split_gemm(rot, cent, metric), rot, cent, metric, D)
    assert worst < 0.5


def _faults(rot, cent, metric):
    D = rot.shape[1]
    A = _rows(rot, cent, metric)
    nq, nl = A.shape
    out = {}
    out["one_slab_missing"] = _rows(rot, cent, metric, slice(96, 128))
    out["last_slab_missing"] = _rows(rot, cent, metric, slice(D - 32, D))
    if metric == 0:
        q, c = rot.astype(np.float64), cent.astype(np.float64)
        out["norms_twice"] = (A + ((q * q).sum(1)[:, None] + (c * c).sum(1)[None, :])).astype(np.float32)
        out["norms_missing"] = (A - ((q * q).sum(1)[:, None] + (c * c).sum(1)[None, :])).astype(np.float32)
    out["stale_row_2A"] = (2.0 * A.astype(np.float64)).astype(np.float32)
    # a 64 x 64 tile edge: query 63 gets list 64's neighbour value (a column off by one at the edge)
    e = A.copy()
    e[63, 64] = A[63, 63]
    out["tile_edge_entry"] = e
    e = A.copy()
    e[nq - 1, nl - 1] = A[nq - 1, nl - 2]  # the last entry of a ragged tile
    out["ragged_corner_entry"] = e
    # split-K over 4 parts of 2 slabs: part 2 dropped; part 0 dropped (it also carries the norms, for L2)
    out["splitk_part2_missing"] = _rows(rot, cent, metric, slice(128, 192))
    p0 = _rows(rot, cent, metric, slice(0, 64)).astype(np.float64)
    if metric == 0:
        q, c = rot.astype(np.float64), cent.astype(np.float64)
        p0 -= (q * q).sum(1)[:, None] + (c * c).sum(1)[None, :]
    out["splitk_part0_missing"] = p0.astype(np.float32)
    e = A.copy()
    e[5, 7] = np.nan
    out["nan_entry"] = e
    out["zeros"] = np.zeros_like(A)
    return out


@pytest.mark.parametrize("metric", [0, 1])
def test_checker_rejects_faulty_rows(operands, metric):
    rot, cent = operands
    D = rot.shape[1]
    faults = _faults(rot, cent, metric)
    for name, A in faults.items():
        worst, bad, _ = rb.check_rows(A, rot, cent, metric, D, skip_rewritten=True)
        assert bad and worst > 1.0, f"{name}: accepted (worst ratio {worst})"
    # the single-entry faults are caught at exactly their entry
    assert rb.check_rows(faults["tile_edge_entry"], rot, cent, metric, D)[1] == [(63, 64)]
    nq, nl = faults["zeros"].shape
    assert rb.check_rows(faults["ragged_corner_entry"], rot, cent, metric, D)[1] == [(nq - 1, nl - 1)]


def test_ip_exemption_is_bitwise(operands):
    """An IP entry the selection rewrote with its canonical L2 distance is left out; the same entry one ulp off is not.
    Left-out entries do not count towards the worst ratio either."""
    rot, cent = operands
    D = rot.shape[1]
    A = _rows(rot, cent, 1)
    l2 = rb.canonical(rot[3:4], cent[9:10], 0)[0]
    A[3, 9] = l2
    worst, bad, skipped = rb.check_rows(A, rot, cent, 1, D, skip_rewritten=True)
    assert not bad and skipped == 1 and worst < 0.5
    assert rb.check_rows(A, rot, cent, 1, D)[1] == [(3, 9)]  # (not asked to leave anything out)
    A[3, 9] = np.nextafter(l2, np.float32(np.inf))
    assert rb.check_rows(A, rot, cent, 1, D, skip_rewritten=True)[1:] == ([(3, 9)], 0)
    # for L2 nothing is left out
    A2 = _rows(rot, cent, 0)
    A2[3, 9] = rb.canonical(rot[3:4], cent[9:10], 0)[0] * np.float32(2)
    assert rb.check_rows(A2, rot, cent, 0, D, skip_rewritten=True)[1:] == ([(3, 9)], 0)
