"""CPU half of the pruning-bound tests (tests/prune_bound.py): the restatements are pinned to hand-built blocks of known
bits, oracle.list_vectors is pinned to ref_search under every numeric variant, and each checker must REJECT what a broken
summary / select kernel would write — a padded lane in a min/max, min and max swapped, a Cauchy-Schwarz term rounded down,
an lbmin one ulp too high, a head bound one ulp too low, a stream entry with a wrong nvalid or gblock, a missing block."""
import ctypes as C

import numpy as np
import pytest

import oracle
import prune_bound as pb
import rabitq_rs_amd as rq
from conftest import build_index
from fetch_ref import ex_codes as fr_ex_codes
from fetch_ref import sign_bits as fr_sign_bits

F32 = np.float32
VARIANT_MASKS = [0, 1, 2, 4, 6]  # the variants GPU variants are paired with (0, 1, 4, 6: test_gpu_numeric_variant.py) and ex_scalar (2)


def _pack(bits, codes, D, ex_bits):
    """FastScan batch_data (codes part + zero factors) and packed ex codes of n vectors, by the builder's own packers."""
    L = rq.builder.lib()
    n = bits.shape[0]
    nb = (n + 31) // 32
    packed = pb.pack_sign_bits(bits, D)
    batch = np.zeros(nb * pb.record_stride(D), np.uint8)
    for b in range(nb):
        batch[b * pb.record_stride(D):b * pb.record_stride(D) + D * 4] = packed[b * D * 4:(b + 1) * D * 4]
    ex = np.zeros((n, D * ex_bits // 8), np.uint8)
    if ex_bits:
        f = {2: L.rbq_build_pack_ex_code_2bit, 6: L.rbq_build_pack_ex_code_6bit}[ex_bits]
        for v in range(n):
            c = np.ascontiguousarray(codes[v], np.uint16)
            f(c.ctypes.data, ex[v].ctypes.data, D)
    return batch, ex


def _set_factors(batch, D, b, fa, fr, fe):
    s = pb.record_stride(D)
    batch[b * s + D * 4:(b + 1) * s] = np.concatenate([fa, fr, fe]).astype(F32).view(np.uint8)


@pytest.mark.parametrize("D,ex_bits", [(64, 0), (64, 2), (64, 6), (128, 6), (960, 6), (2048, 2)])
def test_decoders_read_known_codes(D, ex_bits):
    """Known random sign bits and ex codes (every 6-bit code value, so codes that straddle 32-bit words in the device layout
    are among them), packed by the builder, come back from block_sign_bits / ex_code_rows and from fetch_ref."""
    rng = np.random.default_rng(D + ex_bits)
    n = 45
    bits = rng.integers(0, 2, (n, D)).astype(np.uint8)
    codes = rng.integers(0, 1 << ex_bits, (n, D)).astype(np.uint32) if ex_bits else np.zeros((n, D), np.uint32)
    if ex_bits == 6:
        codes[0, :64] = np.arange(64)
    batch, ex = _pack(bits, codes, D, ex_bits)
    got = np.concatenate([pb.block_sign_bits(batch, D, b) for b in range(2)])[:n]
    assert np.array_equal(got, bits)
    assert np.array_equal(pb.ex_code_rows(ex, D, ex_bits), codes)
    for v in (0, 1, 15, 16, 31, 32, 44):
        assert np.array_equal(fr_sign_bits(batch, D, v), bits[v])
        assert np.array_equal(fr_ex_codes(ex[v], D, ex_bits), codes[v])


def _hand_list(D, ex_bits, n, seed, garbage=True):
    """One list of n vectors with known codes and factors; the padded lanes of the last block hold extreme garbage."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, (n, D)).astype(np.uint8)
    codes = rng.integers(0, 1 << ex_bits, (n, D)).astype(np.uint32) if ex_bits else np.zeros((n, D), np.uint32)
    batch, ex = _pack(bits, codes, D, ex_bits)
    nb = (n + 31) // 32
    fa = rng.standard_normal(nb * 32).astype(F32) * F32(10)
    fr = rng.standard_normal(nb * 32).astype(F32)
    fe = np.abs(rng.standard_normal(nb * 32)).astype(F32)
    if garbage and n % 32:
        pad = np.arange(n, nb * 32)
        fa[pad] = np.where(pad % 2, F32(-3e38), F32(np.inf))
        fr[pad] = np.where(pad % 3 == 0, F32(np.nan), F32(1e30))
        fe[pad] = F32(-np.inf)
    for b in range(nb):
        _set_factors(batch, D, b, fa[32 * b:32 * b + 32], fr[32 * b:32 * b + 32], fe[32 * b:32 * b + 32])
    cent = rng.standard_normal(D).astype(F32)
    fax = rng.standard_normal(n).astype(F32) if ex_bits else np.zeros(n, F32)
    frx = rng.standard_normal(n).astype(F32) if ex_bits else np.zeros(n, F32)
    lst = {"centroid": cent, "ids": np.arange(n, dtype=np.uint64), "batch_data": batch, "ex_codes": ex,
           "f_add_ex": fax, "f_rescale_ex": frx}
    return lst, bits, codes, (fa[:n], fr[:n], fe[:n])


@pytest.mark.parametrize("D,ex_bits,n", [(64, 0, 5), (64, 6, 33), (128, 2, 64), (192, 6, 1), (960, 6, 31), (64, 6, 0)])
def test_restatement_of_hand_built_blocks(D, ex_bits, n):
    """bsum / lsum are exact min / max over the REAL lanes (the padded garbage is ignored); the bsumx terms are the
    f64 Cauchy-Schwarz quantities of the k_list_summaries header, written out per vector from the known codes."""
    lst, bits, codes, (fa, fr, fe) = _hand_list(D, ex_bits, n, seed=D + n + ex_bits)
    r = pb.restate([lst], D, ex_bits)
    nb = (n + 31) // 32
    assert r.bsum.shape == (nb, 6) and list(r.gb0) == [0]
    if n == 0:
        assert not r.lsum_ok[0] and (r.lsum[0] == 0).all()
        return
    for b in range(nb):
        s = slice(32 * b, min(n, 32 * b + 32))
        assert r.bsum_ok[b]
        assert np.array_equal(r.bsum[b], [fa[s].min(), fa[s].max(), fr[s].min(), fr[s].max(), fe[s].min(), fe[s].max()])
        cent = lst["centroid"].astype(np.float64)
        Sx, Bx, S1x, B1x = [], [], [], []
        for v in range(s.start, s.stop):
            u = ((bits[v].astype(np.int64) << ex_bits) + codes[v]).astype(np.float64) - ((1 << ex_bits) - 0.5)
            Sx.append(float(lst["f_add_ex"][v]) + float(lst["f_rescale_ex"][v]) * float(np.dot(cent, u)))
            Bx.append(abs(float(lst["f_rescale_ex"][v])) * float(np.sqrt(np.dot(u, u))))
            S1x.append(float(fa[v]) + float(fr[v]) * float(np.dot(cent, bits[v] - 0.5)))
            B1x.append(abs(float(fr[v])) * np.sqrt(D) / 2)
        want = np.array([max(Sx), max(Bx), max(S1x), max(B1x)])
        assert np.all(np.abs(r.bsumx[b] - want) <= r.tol[b] + 1e-300), (r.bsumx[b], want)
        assert np.array_equal(r.bsumx_abs[b], [np.abs(lst["f_add_ex"][s]).max(), np.abs(lst["f_rescale_ex"][s]).max()])
    assert r.lsum_ok[0] and np.array_equal(r.lsum[0], [fa.min(), fa.max(), fr.min(), fr.max(), fe.min(), fe.max()])


def test_non_finite_factor_makes_block_and_list_unusable():
    lst, _, _, _ = _hand_list(64, 6, 40, seed=3, garbage=False)
    fa, fr, fe = pb.block_factors(lst["batch_data"], 64, 1)
    fa[3] = F32(np.inf)
    _set_factors(lst["batch_data"], 64, 1, fa, fr, fe)
    lst["f_rescale_ex"][0] = F32(np.nan)
    r = pb.restate([lst], 64, 6)
    assert list(r.bsum_ok) == [True, False] and not r.lsum_ok[0]
    assert list(r.bsumx_ok) == [False, False]


def _device_like(r):
    """What a correct summary kernel writes for a Restated: raw [n][8] f32 words of bsum / lsum / bsumx (terms rounded up
    to f32 plus one ulp, as k_list_summaries does)."""
    def rows(vals, ok):
        raw = np.zeros((len(ok), 8), F32)
        raw[:, :6] = np.where(ok[:, None], vals, 0)
        raw[:, 6] = ok.astype(np.uint32).view(F32)
        return raw

    up32 = pb.up32
    x = np.zeros((len(r.bsumx_ok), 6), F32)
    for g in range(len(r.bsumx_ok)):
        x[g, :4] = [up32(v) for v in r.bsumx[g]]
        x[g, 4:] = r.bsumx_abs[g]
    return rows(r.bsum, r.bsum_ok), rows(r.lsum, r.lsum_ok), rows(x, r.bsumx_ok)


@pytest.fixture(scope="module")
def small():
    data, built = build_index(n=700, dim=64, nlist=6, total_bits=7, metric=0, rotator=1, seed=77)
    lists = pb.lists_of(built)
    r = pb.restate(lists, 64, 6)
    yield data, built, lists, r
    built.close()


def test_check_summaries_rejects_broken_summaries(small):
    _, built, lists, r = small
    bsum, lsum, bsumx = _device_like(r)
    viol, worst = pb.check_summaries(r, bsum, lsum, bsumx)
    assert viol == [] and worst <= 3
    # a padded lane counted: the last (partial) block's ranges over all 32 lanes
    c = int(np.nonzero(built.list_sizes() % 32)[0][0])
    n = int(built.list_sizes()[c])
    g = int(r.gb0[c]) + (n - 1) // 32
    fa, fr, fe = pb.block_factors(lists[c]["batch_data"], 64, (n - 1) // 32)
    fa[n % 32:] = F32(-1e30)  # (the padded lanes of a reference record hold zeros; a kernel reading them sees whatever is there)
    bad = bsum.copy()
    bad[g, 0] = min(fa.min(), bad[g, 0])
    assert any("fadd_min" in v for v in pb.check_summaries(r, bad, lsum, bsumx)[0])
    fa0, fr0, fe0 = pb.block_factors(lists[c]["batch_data"], 64, (n - 1) // 32)
    bad = bsum.copy()
    bad[g, 4] = min(fe0.min(), bad[g, 4])  # the zero f_error of a padded lane
    assert any("ferr_min" in v for v in pb.check_summaries(r, bad, lsum, bsumx)[0])
    # min and max swapped
    for what in ("bsum", "lsum"):
        arr = {"bsum": bsum, "lsum": lsum}[what].copy()
        arr[0, [2, 3]] = arr[0, [3, 2]]
        args = (arr, lsum, bsumx) if what == "bsum" else (bsum, arr, bsumx)
        assert any(v.startswith(f"{what}[0].fres") for v in pb.check_summaries(r, *args)[0]), what
    # a usable flag cleared / set
    bad = bsum.copy()
    bad[1, 6] = np.uint32(0).view(F32)
    assert pb.check_summaries(r, bad, lsum, bsumx)[0]
    # S (and each other term) rounded down: the f32 just below its f64 value
    for k in range(3):  # (B1 = |f_rescale| sqrt(D) / 2 is exact in f32 at D = 64)
        g = int(np.nonzero([F32(v) != v for v in r.bsumx[:, k]])[0][0])
        bad = bsumx.copy()
        f = F32(r.bsumx[g, k])
        bad[g, k] = f if float(f) < r.bsumx[g, k] else np.nextafter(f, F32(-np.inf))
        assert any("below its f64 value" in v for v in pb.check_summaries(r, bsum, lsum, bad)[0]), k
    # rounded to nearest and then one ulp up: never below the f64 value, but not k_list_summaries' rounding
    g = int(np.nonzero([F32(v) != v and F32(v) < v for v in r.bsumx[:, 0]])[0][0])
    bad = bsumx.copy()
    bad[g, 0] = np.nextafter(F32(r.bsumx[g, 0]), F32(np.inf))
    assert any("up32" in v for v in pb.check_summaries(r, bsum, lsum, bad)[0])
    # more than 3 ulp above it
    bad = bsumx.copy()
    for _ in range(3):
        bad[2, 1] = np.nextafter(bad[2, 1], F32(np.inf))
    assert any("ulp above" in v for v in pb.check_summaries(r, bsum, lsum, bad)[0])
    # an |f_add_ex| maximum that is not exact
    bad = bsumx.copy()
    bad[0, 4] = np.nextafter(bad[0, 4], F32(np.inf))
    assert any("fadd_ex_abs" in v for v in pb.check_summaries(r, bsum, lsum, bad)[0])


def _replay(built, q, top_k, nprobe):
    """ref_search rebuilt from oracle.list_vectors: the reference's skip rule, then ref_heap_trace over the pushes."""
    rqv = oracle.rotate(built, q)
    qc = oracle.query_precompute(rqv, built.header.ex_bits)
    cids = oracle.select_probes(built, rqv, nprobe)
    pushed_d, pushed_i, best = [], [], []
    skipped = ext = 0
    for cid in cids:
        g_add, g_err = oracle.probe_geometry(built, rqv, cid)
        v = oracle.list_vectors(built, rqv, cid, g_add, g_err)
        ids = built.list_ids(cid)
        dot = F32(-g_add) if built.header.metric == 1 else None
        for i in range(len(ids)):
            lower = v["lb"][i]
            if not np.isfinite(lower):
                lower = F32(0.0) if built.header.metric == 0 else -(dot + F32(qc.query_norm))
            distk = np.inf if len(best) < top_k else best[top_k - 1]
            if lower >= distk:
                skipped += 1
                continue
            ext += built.header.ex_bits > 0
            d = v["dist"][i]
            if not np.isfinite(d):
                continue
            pushed_d.append(d)
            pushed_i.append(ids[i])
            best = sorted(best + [float(d)])[:top_k]
    d = np.array(pushed_d, F32)
    i = np.array(pushed_i, np.uint64)
    oid, odist, n = np.zeros(top_k, np.uint64), np.zeros(top_k, F32), C.c_uint32()
    assert oracle.lib().ref_heap_trace(d.ctypes.data, i.ctypes.data, len(d), top_k, oid.ctypes.data, odist.ctypes.data,
                                       C.byref(n)) == 0
    sc = odist[:n.value] if built.header.metric == 0 else -odist[:n.value]
    return oid[:n.value], sc, (len(pushed_d), skipped, ext)


@pytest.mark.parametrize("bits,metric", [(7, 0), (3, 1), (1, 0)])
def test_list_vectors_reproduce_ref_search_under_every_variant(bits, metric):
    data, built = build_index(n=900, dim=96, nlist=8, total_bits=bits, metric=metric, rotator=1, seed=bits * 10 + metric)
    rng = np.random.default_rng(bits)
    q = data[rng.choice(len(data), 6, replace=False)] + F32(0.05) * rng.standard_normal((6, 96)).astype(F32)
    top_k, nprobe = 10, 4
    try:
        for mask in VARIANT_MASKS:
            with oracle.variant(mask):
                rc, ids, sc, cnt, diag = oracle.search_batch(built, q, top_k, nprobe, want_diag=True, nthreads=1)
                assert rc == 0
                for i in range(len(q)):
                    rid, rsc, dg = _replay(built, q[i], top_k, nprobe)
                    assert np.array_equal(rid, ids[i, :cnt[i]]), (mask, i)
                    assert np.array_equal(rsc.view(np.uint32), sc[i, :cnt[i]].view(np.uint32)), (mask, i)
                    assert tuple(int(x) for x in diag[i]) == dg, (mask, i)
    finally:
        built.close()


def _plan_and_stream(built, lists, r, q, nprobe):
    rqv = oracle.rotate(built, q)
    cids = oracle.select_probes(built, rqv, nprobe)
    plan = pb.probe_plan(built, lists, r, rqv, cids, oracle)
    items = []
    for rank, p in enumerate(plan):
        for b in range((p["n"] + 31) // 32):
            nv = min(32, p["n"] - 32 * b)
            lb = p["lb"][32 * b:32 * b + nv]
            L = lb.min() if p["fin"][32 * b:32 * b + nv].all() else F32(-np.inf)
            items.append([p["gb0"] + b, (rank << 6) | nv, np.array([L], F32).view(np.uint32)[0], 0])
    return plan, np.array(items, np.uint32), list(cids)


def test_check_stream_rejects_broken_streams(small):
    data, built, lists, r = small
    plan, items, cids = _plan_and_stream(built, lists, r, data[3] + 0.01, 4)
    viol, st = pb.check_stream(items, cids, plan)
    assert viol == [] and st.entries == len(items) and st.sharp == st.finite
    # lbmin one ulp above the block's smallest lb_v
    bad = items.copy()
    bad[1, 2] = np.array([np.nextafter(bad[1:2, 2].view(F32)[0], F32(np.inf))], F32).view(np.uint32)[0]
    assert any("> min lb_v" in v for v in pb.check_stream(bad, cids, plan)[0])
    # a finite lbmin where a factor is not finite
    plan2 = [dict(p) for p in plan]
    plan2[0]["fin"] = plan2[0]["fin"].copy()
    plan2[0]["fin"][0] = False
    assert any("not finite" in v for v in pb.check_stream(items, cids, plan2)[0])
    # wrong nvalid, wrong gblock, wrong rank
    for col, delta in ((1, -1), (0, 1), (1, 64)):
        bad = items.copy()
        k = int(np.nonzero((items[:, 1] & 63) < 32)[0][0]) if col == 1 and delta == -1 else 0
        bad[k, col] = bad[k, col] + np.uint32(delta) if delta > 0 else bad[k, col] - np.uint32(1)
        assert any("expected" in v for v in pb.check_stream(bad, cids, plan)[0]), (col, delta)
    # a missing block, an extra entry
    assert pb.check_stream(np.delete(items, 2, axis=0), cids, plan)[0]
    assert pb.check_stream(items[:-1], cids, plan)[0]
    assert any("beyond" in v for v in pb.check_stream(np.vstack([items, items[-1:]]), cids, plan)[0])
    # the probe order: a swapped pair (eager), a dropped list accepted only when it is reported as dropped
    assert pb.check_stream(items, [cids[1], cids[0]] + cids[2:], plan)[0]
    n0 = (plan[0]["n"] + 31) // 32
    lazy_items = items[n0:].copy()
    lazy_items[:, 1] -= np.uint32(64)
    assert pb.check_stream(lazy_items, cids[1:], plan, eager=False)[0] == []
    assert pb.check_stream(lazy_items, cids[1:], plan, eager=False, dropped=[cids[0]])[0] == []
    assert pb.check_stream(lazy_items, cids[1:], plan, eager=False, dropped=[])[0]


def test_check_consts_rejects_ranges_that_miss_a_vector(small):
    data, built, lists, r = small
    rqv = oracle.rotate(built, data[5])
    lut, delta, sum_vl = oracle.query_lut(rqv)
    amin, amax = pb.lut_range(lut)
    accu = np.concatenate([oracle.list_vectors(built, rqv, c, 0.0, 0.0)["accu"] for c in range(6)])
    ex = np.concatenate([oracle.list_vectors(built, rqv, c, 0.0, 0.0)["exdot"] for c in range(6)])
    q1 = float(np.abs(rqv.astype(np.float64)).sum())
    c = np.zeros(12, F32)
    c[pb.QC["amin"]], c[pb.QC["amax"]] = amin, amax
    c[pb.QC["exlo"]], c[pb.QC["exhi"]] = ex.min(), ex.max()
    c[pb.QC["q1norm"]] = F32(q1 * 1.001)
    assert pb.check_consts(c, rqv, accu, ex) == [] and pb.check_consts(c, rqv, accu, ex, lut) == []
    for k, v in (("amin", amin - 1), ("amax", amax + 1)):  # a range wider than the LUT allows covers every accu: only the LUT sees it
        bad = c.copy()
        bad[pb.QC[k]] = v
        assert pb.check_consts(bad, rqv, accu, ex) == [] and pb.check_consts(bad, rqv, accu, ex, lut), k
    for k, v in (("amin", accu.min() + 1), ("amax", accu.max() - 1), ("exlo", np.nextafter(ex.min(), F32(np.inf))),
                 ("exhi", np.nextafter(ex.max(), F32(-np.inf))), ("q1norm", F32(q1 * 0.9999)), ("q1norm", F32(q1 * 1.01))):
        bad = c.copy()
        bad[pb.QC[k]] = v
        assert pb.check_consts(bad, rqv, accu, ex), k


def test_check_head_ub_rejects_a_low_bound_and_a_wrong_t_ub():
    rng = np.random.default_rng(9)
    blocks, cands = {}, []
    for gb in range(12):
        nv = 32 if gb % 5 else 7
        dist = (rng.random(nv) * 10).astype(F32)
        lb = (dist - rng.random(nv).astype(F32)).astype(F32)
        blocks[gb] = (dist, lb)
        cands.append((gb, F32(dist.max() * F32(1.5)), nv))
    cands.append((12, F32(np.inf), 32))
    blocks[12] = (np.zeros(32, F32), np.zeros(32, F32))
    t = pb.t_ub_rule([c[1] for c in cands], [c[2] for c in cands], 40)
    viol, st = pb.check_head_ub(cands, blocks, t, 40)
    assert viol == [] and st["finite"] == 12 and 1.4 < st["median_ratio"] < 1.6
    # U one ulp below a vector's distance
    bad = list(cands)
    gb, _, nv = bad[3]
    bad[3] = (gb, np.nextafter(blocks[gb][0].max(), F32(-np.inf)), nv)
    assert any("< max(dist_v, lb_v)" in v for v in pb.check_head_ub(bad, blocks, pb.t_ub_rule([c[1] for c in bad], [c[2] for c in bad], 40), 40)[0])
    # ... or below a lower bound that exceeds its distance
    d, lb = blocks[4]
    blocks2 = dict(blocks)
    blocks2[4] = (d, np.where(np.arange(len(d)) == 0, cands[4][1] * F32(2), lb).astype(F32))
    assert pb.check_head_ub(cands, blocks2, t, 40)[0]
    # wrong nvalid; T_ub one ulp off the rule
    bad = list(cands)
    bad[0] = (bad[0][0], bad[0][1], bad[0][2] - 1)
    assert pb.check_head_ub(bad, blocks, t, 40)[0]
    assert any("T_ub" in v for v in pb.check_head_ub(cands, blocks, np.nextafter(t, F32(-np.inf)), 40)[0])
    assert pb.t_ub_rule([F32(1), F32(2)], [3, 3], 7) == np.inf


def test_extreme_bits_reach_the_lut_range(small):
    """The sharp GPU case's codes: per codebook the argmin (argmax) nibble of the query's LUT gives accu == amin (amax),
    confirmed by the reference's own accumulate."""
    data, built, lists, r = small
    rqv = oracle.rotate(built, data[1])
    lut, _, _ = oracle.query_lut(rqv)
    amin, amax = pb.lut_range(lut)
    for lowest in (True, False):
        bits = pb.extreme_bits(lut, lowest)[None, :]
        codes = pb.pack_sign_bits(bits, 64)
        accu = np.zeros(32, np.uint16)
        oracle.lib().ref_accumulate_batch(codes.ctypes.data, lut.ctypes.data, 64, accu.ctypes.data)
        assert int(accu[0]) == (amin if lowest else amax)
