"""CPU side of the one-product f16 ranking GEMM's error budget (tests/rank_f16_bound.py): the image is pinned to hand-written
bit patterns, the residual is shown to be exact in f32, and qh.ch accumulated in f32 in several orders is held to the budget
against float64 over ordinary data, data scaled by 1e-4 and 1e4, integer data, per-coordinate scales 1e-3 .. 1e3 and inputs
with subnormal and flushed elements.  A row with one K slab left out, and a row whose budget ignores the flush, are rejected."""
import numpy as np
import pytest

import rank_bound as rb
import rank_f16_bound as fb
from conftest import make_dataset


def _bits(u):
    return np.array(u, dtype=np.uint32).view(np.float32)


# (x bits, image bits)
IMAGE_KAT = [
    (0x3F800000, 0x3C00),  # 1.0
    (0xBF800000, 0xBC00),
    (0x3F801000, 0x3C00),  # 1 + 2^-11: a tie, DOWN to the even 0x3C00
    (0x3F803000, 0x3C02),  # 1 + 3 * 2^-11: a tie, UP to the even 0x3C02
    (0x3F801001, 0x3C01),  # just above the tie
    (0x477FE000, 0x7BFF),  # 65504, the largest half
    (0x477FEFFF, 0x7BFF),  # just below the tie to 2^16
    (0x477FF000, 0x7C00),  # 65520: the tie goes to the even 2^16 = inf
    (0xC77FF000, 0xFC00),
    (0x7F800000, 0x7C00),  # inf
    (0x38800000, 0x0400),  # 2^-14, the smallest normal half
    (0x387FE000, 0x0400),  # 2^-14 - 2^-25: a tie at the subnormal spacing, UP to the even 2^-14 — stays
    (0x387FDFFF, 0x0000),  # just below: the subnormal 1023 * 2^-24 — flushed
    (0x38000000, 0x0000),  # 2^-15 — flushed
    (0xB8000000, 0x8000),  # -2^-15 — flushed, the sign stays
    (0x33800000, 0x0000),  # 2^-24, the smallest subnormal half — flushed
    (0x00000001, 0x0000),  # smallest f32 subnormal
    (0x00000000, 0x0000),
    (0x80000000, 0x8000),
]


def test_image_known_answers():
    x = _bits([k[0] for k in IMAGE_KAT])
    got = fb.f16_image(x)
    for (xb, want), g in zip(IMAGE_KAT, got):
        assert int(g) == want, f"x={xb:#010x}: image {int(g):#06x}, want {want:#06x}"
    nan = fb.f16_image(_bits([0x7FC00000, 0xFFC00001]))
    assert ((nan & 0x7C00) == 0x7C00).all() and ((nan & 0x03FF) != 0).all()


def test_image_never_subnormal_and_residual_exact_in_f32():
    """No stored half is subnormal; x - f16(x) evaluated in f32 equals the float64 difference bit for bit, flushed elements
    included (the residual is then x itself)."""
    rng = np.random.default_rng(11)
    u = rng.integers(0x00000001, 0x47000000, 400000, dtype=np.uint64).astype(np.uint32)  # subnormal f32 .. 32768
    u |= rng.integers(0, 2, u.size, dtype=np.uint32) << 31
    x = u.view(np.float32)
    bits = fb.f16_image(x)
    assert (((bits & 0x7C00) != 0) | ((bits & 0x03FF) == 0)).all()
    r32 = x - fb.f16_value(bits)
    r64 = x.astype(np.float64) - fb.f16_value(bits).astype(np.float64)
    assert np.array_equal(r32.astype(np.float64), r64)
    flushed = (bits & 0x7FFF) == 0
    assert flushed.any() and np.array_equal(r32[flushed].view(np.uint32) & 0x7FFFFFFF, x[flushed].view(np.uint32) & 0x7FFFFFFF)
    kept = ~flushed
    assert (np.abs(r64[kept]) <= 2.0 ** -11 * np.abs(x[kept].astype(np.float64))).all()


def test_residual_rounding_and_gate():
    x = make_dataset(300, 192, 16, 5)
    bits = fb.f16_image(x)
    assert fb.residual_ok(fb.resid32(x, bits), fb.resid64(x, bits)).all()
    cn2 = (x.astype(np.float64) ** 2).sum(1).astype(np.float32)
    assert fb.gate(fb.resid32(x, bits), cn2)
    # flushed halves: the residual is a large part of the norm
    s = (x * np.float32(1e-4)).astype(np.float32)
    sb = fb.f16_image(s)
    assert (((sb & 0x7FFF) == 0) & (s != 0)).any()
    assert not fb.gate(fb.resid32(s, sb), (s.astype(np.float64) ** 2).sum(1).astype(np.float32))
    # halves that are not finite
    b = (x * np.float32(1e5)).astype(np.float32)
    bb = fb.f16_image(b)
    assert ((bb & 0x7FFF) == 0x7C00).any()
    r = fb.resid32(b, bb)
    assert not np.isfinite(r).all() and not fb.gate(r, (b.astype(np.float64) ** 2).sum(1).astype(np.float32))
    # a residual that is not finite never passes as a measured one
    assert not fb.residual_ok(np.float32([1.0]), np.array([np.inf])).any()
    assert not fb.residual_ok(np.float32([0.999999]), np.array([1.0])).any()
    assert not fb.residual_ok(np.float32([1.0001]), np.array([1.0])).any()


def test_select_eps_matches_formula():
    D, qn2, cm2, rq = 960, np.float32(933.5), np.float32(1011.25), np.float32(6.5e-3)
    cmax, rc = fb.cnorm_max_of([cm2]), np.float32(7.1e-3)
    want = ((6 * D + 16) * 2.0 ** -24 * (float(qn2) + float(cm2))
            + 2.01 * (float(rq) * float(cmax) + (np.sqrt(float(qn2)) + float(rq)) * float(rc))) * 1.001
    got = float(fb.select_eps(D, qn2, cm2, rq, cmax, rc))
    assert abs(got - want) <= 1e-6 * want
    assert float(cmax) >= np.sqrt(float(cm2)) and float(cmax) <= np.sqrt(float(cm2)) * (1 + 1e-5)
    assert not np.isfinite(fb.select_eps(D, qn2, cm2, np.float32(np.inf), cmax, rc))


# ---- the budget against float64 -----------------------------------------------------------------------------------

def _inputs(kind, nq, nl, D, seed):
    q, c = make_dataset(nq, D, 16, seed), make_dataset(nl, D, 16, seed + 1)
    f = np.float32
    if kind == "mix":
        return q, c
    if kind == "mix_1e-4":
        return (q * f(1e-4)).astype(f), (c * f(1e-4)).astype(f)
    if kind == "mix_1e4":
        return (q * f(1e4)).astype(f), (c * f(1e4)).astype(f)
    if kind == "int255":
        rng = np.random.default_rng(seed)
        return rng.integers(0, 256, (nq, D)).astype(f), rng.integers(0, 256, (nl, D)).astype(f)
    if kind == "coord_scales":
        s = np.logspace(-3, 3, D, dtype=f)[None, :]
        return (q * s).astype(f), (c * s).astype(f)
    if kind == "subnormal":  # ordinary rows with a third of the elements in the subnormal / flushed range of f16
        rng = np.random.default_rng(seed)
        tiny = f(2.0) ** rng.integers(-30, -13, D).astype(f)
        sq = np.where(rng.random(D) < 0.33, tiny, f(1.0))[None, :]
        sc = np.where(rng.random(D) < 0.33, tiny, f(1.0))[None, :]
        return (q * sq).astype(f), (c * sc).astype(f)
    raise ValueError(kind)


def _dot32(qh, ch, order):
    """qh.ch with f32 accumulation in the given K order (products of two halves are exact in f32)."""
    acc = np.zeros((qh.shape[0], ch.shape[0]), np.float32)
    for k in order:
        acc = acc + qh[:, k, None] * ch[None, :, k]
    return acc


def _orders(D, seed):
    fwd = np.arange(D)
    yield "forward", [fwd]
    yield "reverse", [fwd[::-1]]
    yield "shuffled", [np.random.default_rng(seed).permutation(D)]
    yield "four partial sums", [fwd[i::4] for i in range(4)]  # (partial accumulators combined at the end)


def _score(dot32, rot, cent, metric):
    if metric == 1:
        return dot32
    qn = np.zeros(rot.shape[0], np.float32)
    for k in range(rot.shape[1]):  # (the preparation's sequential f32 sum)
        qn = qn + rot[:, k] * rot[:, k]
    cn = (cent.astype(np.float64) ** 2).sum(1).astype(np.float32)
    s = (qn[:, None] + cn[None, :]).astype(np.float32)
    return (s.astype(np.float64) - 2.0 * dot32.astype(np.float64)).astype(np.float32)  # (fmaf: one rounding)


def _gemm(rot, cent, metric, parts, drop=None, flush=True):
    qh, ch = fb.f16_value(fb.f16_image(rot, flush)), fb.f16_value(fb.f16_image(cent, flush))
    dot = np.zeros((rot.shape[0], cent.shape[0]), np.float32)
    for p in parts:
        if drop is not None:
            p = p[(p < drop.start) | (p >= drop.stop)]
        dot = dot + _dot32(qh, ch, p)
    return _score(dot, rot, cent, metric)


KINDS = ["mix", "mix_1e-4", "mix_1e4", "int255", "coord_scales", "subnormal"]


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_budget_holds_in_any_order(kind, metric):
    D = 192
    rot, cent = _inputs(kind, 24, 40, D, 70 + len(kind))
    if kind == "subnormal":
        bits = fb.f16_image(cent)
        assert (((bits & 0x7FFF) == 0) & (cent != 0)).any(), "no flushed element in the subnormal inputs"
    for name, parts in _orders(D, 3):
        A = _gemm(rot, cent, metric, parts)
        worst, bad, _ = fb.check_rows(A, rot, cent, metric, D)
        assert not bad and worst <= 1.0, (kind, name, worst, bad[:5])


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("kind", ["mix", "int255", "coord_scales"])
def test_missing_slab_is_rejected(kind, metric):
    """One K slab of 64 left out of the product: far outside the budget wherever the slab carries weight."""
    D = 192
    rot, cent = _inputs(kind, 24, 40, D, 90 + len(kind))
    fwd = [np.arange(D)]
    for slab in ((2,) if kind == "coord_scales" else (0, 2)):  # (coord_scales: slab 0 holds the coordinates scaled by 1e-3 .. 1e-1)
        A = _gemm(rot, cent, metric, fwd, drop=slice(64 * slab, 64 * slab + 64))
        worst, bad, _ = fb.check_rows(A, rot, cent, metric, D)
        assert bad and worst > 1.0, (kind, slab, worst)
    e = _gemm(rot, cent, metric, fwd)
    e[5, 7] = np.nan
    assert fb.check_rows(e, rot, cent, metric, D)[1] == [(5, 7)]


@pytest.mark.parametrize("metric", [0, 1])
def test_flush_must_be_accounted_for(metric):
    """Centroid elements in f16's subnormal range against unit query elements: the stored image holds zeros there, and a
    budget whose residuals are taken from the UNFLUSHED halves rejects the very row the GEMM computes; the budget of the
    stored bits accepts it."""
    D = 64
    rot = np.ones((3, D), np.float32)
    cent = np.full((5, D), 3e-5, np.float32)
    A = _gemm(rot, cent, metric, [np.arange(D)])
    worst, bad, _ = fb.check_rows(A, rot, cent, metric, D)
    assert not bad and worst <= 1.0, worst
    unflushed = fb.f16_image(cent, flush=False)
    assert ((unflushed & 0x7FFF) != 0).all() and ((fb.f16_image(cent) & 0x7FFF) == 0).all()
    worst, bad, _ = fb.check_rows(A, rot, cent, metric, D, cbits=unflushed)
    assert len(bad) == A.size and worst > 1.0, worst
    # and the other way round: a GEMM that did multiply the subnormal halves stays inside the budget of ITS image
    B = _gemm(rot, cent, metric, [np.arange(D)], flush=False)
    assert not fb.check_rows(B, rot, cent, metric, D, cbits=unflushed)[1]
