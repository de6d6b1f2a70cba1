"""The scan's pruning bounds restated in numpy, shared by test_gpu_prune_bound.py (which holds the device's summaries,
stream bounds and query constants to them) and test_prune_bound_host.py (which pins the restatements and shows that every
checker rejects what a broken kernel would write).

The summaries are restated from the REFERENCE layout of the codes (a ClusterData's batch_data / ex_codes, or the same
arrays of an RBQ1 stream), never from the device's re-laid blocks, so a relayout bug shows up as well.

  block_sign_bits   the sign bits of all 32 lanes of one FastScan batch record (fetch_ref.sign_bits, 32 lanes at once)
  ex_code_rows      the ex codes of many vectors (fetch_ref.ex_codes, vectorised over vectors)
  restate           BlockSummary (bsum) per block, the list summary (lsum) per list, BlockSummaryEx (bsumx) terms in f64
  check_summaries   device bsum / lsum / bsumx against the restatement
  check_stream      device block stream (StreamItem) against the oracle's probe order and per-vector lower bounds
  check_consts      QueryConsts amin / amax, exlo / exhi, q1norm against every vector seen
  check_head_ub     the head bounds U (block_ub) and T_ub of the lazy selection against the oracle's vectors
"""
import ctypes as C

import numpy as np

from fetch_ref import KPERM0

F32 = np.float32
_INV_KPERM0 = np.argsort(KPERM0)  # _INV_KPERM0[v] = j with KPERM0[j] == v
# QueryConsts (types.hpp) as 12 f32 words
QC = {n: i for i, n in enumerate(("delta", "sum_vl", "k1x", "kbx", "scale", "qnorm", "qnorm2", "exlo", "exhi", "q1norm",
                                   "amin", "amax"))}
Q1NORM_SLACK = 1.001  # the prep kernels' q1norm = (sum of positives - sum of negatives) * 1.001


def record_stride(D):
    return D * 4 + 384


def block_sign_bits(batch, D, b):
    """[32][D] sign bits of the 32 lanes of batch record b (unpack_single_vector: KPERM0 nibble pairing, MSB first)."""
    s = record_stride(D)
    rec = np.asarray(batch, np.uint8)[b * s:b * s + D * 4].reshape(D // 8, 32)
    v = np.arange(32)
    j = _INV_KPERM0[v % 16]
    sh = np.where(v < 16, 0, 4).astype(np.uint8)
    hi = (rec[:, j] >> sh) & 15
    lo = (rec[:, j + 16] >> sh) & 15
    byte = (hi.astype(np.uint32) << 4) | lo
    bits = (byte[:, :, None] >> (7 - np.arange(8))) & 1  # [D/8][32][8]
    return bits.transpose(1, 0, 2).reshape(32, D).astype(np.uint32)


def block_factors(batch, D, b):
    """(f_add, f_rescale, f_error) [32] each of batch record b, padded lanes included."""
    s = record_stride(D)
    f = np.frombuffer(np.asarray(batch, np.uint8)[b * s + D * 4:(b + 1) * s].tobytes(), np.float32)
    return f[:32].copy(), f[32:64].copy(), f[64:96].copy()


def ex_code_rows(packed, D, ex_bits):
    """[n][D] ex codes of n vectors from their packed rows [n][D * ex_bits / 8] (cpp-compat packings, fetch_ref.ex_codes)."""
    p = np.asarray(packed, np.uint8)
    n = p.shape[0]
    out = np.zeros((n, D), np.uint32)
    if ex_bits == 0 or n == 0:
        return out
    if ex_bits == 2:
        w = p.reshape(n, D // 16, 4).astype(np.uint32)
        for i in range(4):  # byte i: bits 2g hold the code of dim 16t + 4g + i
            for g in range(4):
                out[:, 4 * g + i::16] = (w[:, :, i] >> (2 * g)) & 3
        return out
    assert ex_bits == 6, ex_bits
    g12 = p.reshape(n, D // 16, 12).astype(np.uint32)
    for i in range(8):  # bytes 0-7: low nibbles of dims i (low half) and i + 8 (high half)
        out[:, i::16] = g12[:, :, i] & 15
        out[:, i + 8::16] = g12[:, :, i] >> 4
    for i in range(4):  # bytes 8-11: the top two bits, laid out like the 2-bit packing
        for g in range(4):
            out[:, 4 * g + i::16] |= ((g12[:, :, 8 + i] >> (2 * g)) & 3) << 4
    return out


def lists_of(built):
    """The reference-layout arrays of every list of a builder.BuiltIndex (or of a HostIndex)."""
    return [built.list_arrays(c) for c in range(int(built.n_lists))]


class Restated:
    """What the summary kernels must write, restated from the reference layout.
    bsum [nblocks][6] f32 + bsum_ok; lsum [nlist][6] f32 + lsum_ok; bsumx [nblocks][4] f64 (S, B, S1, B1 maxima over the
    block's real vectors) with tol [nblocks][4] (the f64 rounding of the device's own accumulation), bsumx_abs [nblocks][2]
    f32 (largest |f_add_ex|, |f_rescale_ex|) + bsumx_ok; gb0 [nlist] first global block of every list."""


def restate(lists, D, ex_bits):
    nl = len(lists)
    nbs = [(int(len(a["ids"])) + 31) // 32 for a in lists]
    nblk = int(sum(nbs))
    r = Restated()
    r.gb0 = np.concatenate([[0], np.cumsum(nbs)[:-1]]).astype(np.int64) if nl else np.zeros(0, np.int64)
    r.bsum = np.zeros((nblk, 6), F32)
    r.bsum_ok = np.zeros(nblk, bool)
    r.lsum = np.zeros((nl, 6), F32)
    r.lsum_ok = np.zeros(nl, bool)
    r.bsumx = np.zeros((nblk, 4), np.float64)
    r.tol = np.zeros((nblk, 4), np.float64)
    r.bsumx_abs = np.zeros((nblk, 2), F32)
    r.bsumx_ok = np.zeros(nblk, bool)
    centre = (1 << ex_bits) - 0.5
    u64 = 2.0 ** -53
    for c, a in enumerate(lists):
        n = int(len(a["ids"]))
        cent = np.asarray(a["centroid"], np.float64)
        exc = ex_code_rows(a["ex_codes"], D, ex_bits) if ex_bits else None
        fax_all = np.asarray(a["f_add_ex"], F32) if ex_bits else np.zeros(n, F32)
        frx_all = np.asarray(a["f_rescale_ex"], F32) if ex_bits else np.zeros(n, F32)
        for b in range(nbs[c]):
            g = int(r.gb0[c]) + b
            nv = min(32, n - 32 * b)
            fa, fr, fe = (x[:nv] for x in block_factors(a["batch_data"], D, b))
            ok = bool(np.isfinite(fa).all() and np.isfinite(fr).all() and np.isfinite(fe).all())
            r.bsum_ok[g] = ok
            if ok:
                r.bsum[g] = [fa.min(), fa.max(), fr.min(), fr.max(), fe.min(), fe.max()]
            bits = block_sign_bits(a["batch_data"], D, b)[:nv].astype(np.int64)
            code = bits << ex_bits
            if ex_bits:
                code = code + exc[32 * b:32 * b + nv]
            up = code.astype(np.float64) - centre
            ub = bits.astype(np.float64) - 0.5
            fax, frx = fax_all[32 * b:32 * b + nv], frx_all[32 * b:32 * b + nv]
            with np.errstate(invalid="ignore", over="ignore"):
                dcu, dcb = up @ cent, ub @ cent
                S = fax.astype(np.float64) + frx.astype(np.float64) * dcu
                B = np.abs(frx.astype(np.float64)) * np.sqrt((up * up).sum(1))
                S1 = fa.astype(np.float64) + fr.astype(np.float64) * dcb
                B1 = np.abs(fr.astype(np.float64)) * np.sqrt(float(D)) * 0.5
                tS = 4 * (D + 4) * u64 * (np.abs(fax) + np.abs(frx) * (np.abs(up) @ np.abs(cent)))
                tS1 = 4 * (D + 4) * u64 * (np.abs(fa) + np.abs(fr) * (np.abs(ub) @ np.abs(cent)))
                tB = 8 * u64 * B
                tB1 = 8 * u64 * B1
            okx = bool(np.isfinite(fa).all() and np.isfinite(fr).all() and np.isfinite(fax).all() and np.isfinite(frx).all()
                       and np.isfinite(S).all() and np.isfinite(B).all() and np.isfinite(S1).all())
            r.bsumx_ok[g] = okx
            if okx:
                for k, (v, t) in enumerate(((S, tS), (B, tB), (S1, tS1), (B1, tB1))):
                    r.bsumx[g, k] = v.max()
                    r.tol[g, k] = t.max()
                r.bsumx_abs[g] = [np.abs(fax).max(), np.abs(frx).max()]
        if nbs[c] and r.bsum_ok[r.gb0[c]:r.gb0[c] + nbs[c]].all():
            blk = r.bsum[r.gb0[c]:r.gb0[c] + nbs[c]]
            r.lsum_ok[c] = True
            r.lsum[c] = [blk[:, 0].min(), blk[:, 1].max(), blk[:, 2].min(), blk[:, 3].max(), blk[:, 4].min(), blk[:, 5].max()]
    return r


def summary_rows(raw):
    """Device BlockSummary / BlockSummaryEx rows ([n][8] f32 words) -> (values [n][6] f32, usable [n] bool)."""
    raw = np.asarray(raw, F32).reshape(-1, 8)
    return raw[:, :6].copy(), raw[:, 6].view(np.uint32) != 0


def up32(x):
    """k_list_summaries' rounding of an f64 term: up to the next f32 at or above x, then one ulp more."""
    f = np.float32(x)
    if float(f) < x:
        f = np.nextafter(f, np.float32(np.inf))
    return np.nextafter(f, np.float32(np.inf))


def _ulps_above(dev, lo):
    """Number of f32 steps from the largest f32 <= lo (f64) up to dev (f32); negative when dev < lo."""
    lo32 = np.float32(lo)
    if float(lo32) > lo:
        lo32 = np.nextafter(lo32, np.float32(-np.inf))
    a, b = np.array([lo32], F32).view(np.int32)[0], np.array([dev], F32).view(np.int32)[0]
    key = lambda k: int(k) if k >= 0 else -(int(k) & 0x7FFFFFFF)  # noqa: E731  (ordered integer of a float's bits)
    return key(b) - key(a)


def check_summaries(rest, bsum, lsum, bsumx, max_ulps=3):
    """Device bsum [nblocks][8] / lsum [nlist][8] / bsumx [nblocks][8] (raw f32 words) against a Restated.
    Returns (violations: list of str, worst ulps of S, B, S1, B1 above their f64 value)."""
    viol = []
    bv, bok = summary_rows(bsum)
    lv, lok = summary_rows(lsum)
    xv, xok = summary_rows(bsumx)
    if bv.shape[0] != rest.bsum.shape[0] or lv.shape[0] != rest.lsum.shape[0] or xv.shape[0] != rest.bsumx.shape[0]:
        return [f"shape: device {bv.shape[0]} blocks / {lv.shape[0]} lists, restated {rest.bsum.shape[0]} / {rest.lsum.shape[0]}"], 0
    names = ("fadd_min", "fadd_max", "fres_min", "fres_max", "ferr_min", "ferr_max")
    for what, dv, dok, rv, rok in (("bsum", bv, bok, rest.bsum, rest.bsum_ok), ("lsum", lv, lok, rest.lsum, rest.lsum_ok)):
        for i in np.nonzero(dok != rok)[0][:20]:
            viol.append(f"{what}[{i}].usable = {int(dok[i])}, restated {int(rok[i])}")
        both = dok & rok
        # exact values (-0 == +0: fminf may return either zero); an unusable entry must hold zeros
        bad = np.nonzero((both[:, None] & ~(dv == rv)).any(1) | (~dok & ~rok & (dv != 0).any(1)))[0]
        for i in bad[:20]:
            k = int(np.argmax(dv[i] != rv[i]))
            viol.append(f"{what}[{i}].{names[k]} = {dv[i, k]!r}, restated {rv[i, k]!r}")
    for i in np.nonzero(xok != rest.bsumx_ok)[0][:20]:
        viol.append(f"bsumx[{i}].usable = {int(xok[i])}, restated {int(rest.bsumx_ok[i])}")
    worst = 0
    for g in np.nonzero(xok & rest.bsumx_ok)[0]:
        for k, nm in enumerate(("S", "B", "S1", "B1")):
            lo, hi = rest.bsumx[g, k] - rest.tol[g, k], rest.bsumx[g, k] + rest.tol[g, k]
            d = xv[g, k]
            if not float(d) >= lo:
                viol.append(f"bsumx[{g}].{nm} = {d!r} below its f64 value {rest.bsumx[g, k]!r}")
                continue
            u = _ulps_above(d, hi)
            worst = max(worst, _ulps_above(d, rest.bsumx[g, k]))
            if u > max_ulps:
                viol.append(f"bsumx[{g}].{nm} = {d!r} is {u} ulp above its f64 value {rest.bsumx[g, k]!r}")
            elif not up32(lo) <= d <= up32(hi):  # the kernel's own rounding, up to the f64 error of its accumulation order
                viol.append(f"bsumx[{g}].{nm} = {d!r}, k_list_summaries' up32 of {rest.bsumx[g, k]!r} is {up32(rest.bsumx[g, k])!r}")
        for k, nm in enumerate(("fadd_ex_abs", "fres_ex_abs")):
            if xv[g, 4 + k] != rest.bsumx_abs[g, k]:
                viol.append(f"bsumx[{g}].{nm} = {xv[g, 4 + k]!r}, restated {rest.bsumx_abs[g, k]!r}")
    return viol, worst


def probe_plan(built, lists, rest, rq, cids, oracle, g_err_zero=False):
    """Per probed list in the given order: its geometry (oracle g_add / g_err), every vector's values from the oracle
    (oracle.list_vectors, under the active variant) and the finiteness of each vector's factors and lower bound."""
    D = int(built.padded_dim)
    plan = []
    for cid in cids:
        cid = int(cid)
        g_add, g_err = oracle.probe_geometry(built, rq, cid)
        if g_err_zero:
            g_err = F32(0.0)
        vals = oracle.list_vectors(built, rq, cid, g_add, g_err)
        n = len(vals["lb"])
        a = lists[cid]
        fin = np.isfinite(vals["lb"])
        for b in range((n + 31) // 32):
            nv = min(32, n - 32 * b)
            fa, fr, fe = (x[:nv] for x in block_factors(a["batch_data"], D, b))
            fin[32 * b:32 * b + nv] &= np.isfinite(fa) & np.isfinite(fr) & np.isfinite(fe)
        plan.append({"cid": cid, "gb0": int(rest.gb0[cid]), "n": n, "g_add": g_add, "g_err": g_err, "fin": fin, **vals})
    return plan


def stream_items(raw):
    """Device StreamItem rows ([n][4] u32 words) -> (gblock, rank, nvalid, lbmin)."""
    w = np.asarray(raw).view(np.uint32).reshape(-1, 4)
    return w[:, 0].astype(np.int64), (w[:, 1] >> 6).astype(np.int64), (w[:, 1] & 63).astype(np.int64), w[:, 2].view(F32)


class StreamStats:
    def __init__(self):
        self.entries = 0
        self.finite = 0
        self.sharp = 0          # entries whose lbmin equals the smallest lb_v of the block
        self.worst_gap = 0.0    # largest min_v lb_v - lbmin
        self.worst_rel = 0.0    # ... relative to max(|min_v lb_v|, |lbmin|)

    def add(self, other):
        self.entries += other.entries
        self.finite += other.finite
        self.sharp += other.sharp
        self.worst_gap = max(self.worst_gap, other.worst_gap)
        self.worst_rel = max(self.worst_rel, other.worst_rel)


def check_stream(items, scanned, plan, eager=True, dropped=None):
    """One query's block stream against the oracle.
    items: its StreamItem rows (nstream of them); scanned: the list ids of the probes it names (ProbeInfo.cid of ranks
    0..); plan: probe_plan() in the ORACLE's probe order.  eager: every probed list is scanned, in the oracle's order;
    else the scanned lists are the oracle's order with some lists left out (`dropped`, when given, must be exactly
    those).  Every entry must be block b of its list with rank r and the right number of real vectors, and its lbmin must
    be <= lb_v of every real vector (-inf where a factor or an lb_v is not finite).  Returns (violations, StreamStats)."""
    viol, st = [], StreamStats()
    gblock, rank, nvalid, lbmin = stream_items(items)
    order = [p["cid"] for p in plan]
    scanned = [int(c) for c in scanned]
    if eager and scanned != order:
        viol.append(f"scanned lists {scanned[:8]}... differ from the oracle's probe order {order[:8]}...")
        return viol, st
    if dropped is not None:  # (the selection may also report dead lists outside the probe set)
        missing, dropped = set(order) - set(scanned), set(int(c) for c in dropped)
        if not missing <= dropped or dropped & set(scanned):
            viol.append(f"lists left out of the stream {sorted(missing)[:8]} are not the ones reported dropped {sorted(dropped)[:8]}")
    pos, j = 0, 0
    for r, cid in enumerate(scanned):
        while j < len(plan) and plan[j]["cid"] != cid:
            j += 1
        if j == len(plan):
            viol.append(f"rank {r}: list {cid} is not next in the oracle's probe order")
            return viol, st
        p = plan[j]
        j += 1
        n = p["n"]
        for b in range((n + 31) // 32):
            if pos >= len(gblock):
                viol.append(f"stream ends before block {b} of list {cid} (rank {r})")
                return viol, st
            nv = min(32, n - 32 * b)
            if gblock[pos] != p["gb0"] + b or rank[pos] != r or nvalid[pos] != nv:
                viol.append(f"entry {pos}: (gblock {gblock[pos]}, rank {rank[pos]}, nvalid {nvalid[pos]}), expected "
                            f"({p['gb0'] + b}, {r}, {nv})")
                return viol, st
            lb = p["lb"][32 * b:32 * b + nv]
            fin = p["fin"][32 * b:32 * b + nv]
            L = lbmin[pos]
            st.entries += 1
            if not fin.all():
                if not L == -np.inf:
                    viol.append(f"entry {pos} (list {cid} block {b}): lbmin {L!r} where a factor or lb_v is not finite")
            elif not L <= lb.min():
                viol.append(f"entry {pos} (list {cid} block {b}): lbmin {L!r} > min lb_v {lb.min()!r}")
            elif np.isfinite(L):
                st.finite += 1
                m = float(lb.min())
                gap = m - float(L)
                st.sharp += int(gap == 0.0)
                st.worst_gap = max(st.worst_gap, gap)
                st.worst_rel = max(st.worst_rel, gap / max(abs(m), abs(float(L)), 1e-30))
            pos += 1
    if pos != len(gblock):
        viol.append(f"{len(gblock) - pos} stream entries beyond the probed lists' blocks")
    return viol, st


def check_consts(consts, rq, accu=(), exdot=(), lut8=None):
    """One query's QueryConsts (12 f32 words) against the rotated query (q1norm) and the accu / ex-code dot of every vector
    seen; with the query's u8 LUT given, amin / amax must also equal lut_range(lut8) exactly (a range wider than the codes
    can reach would weaken every block bound silently).  Returns a list of violations."""
    c = np.asarray(consts, F32).reshape(-1)
    viol = []
    if lut8 is not None:
        want = lut_range(lut8)
        if (float(c[QC["amin"]]), float(c[QC["amax"]])) != (float(want[0]), float(want[1])):
            viol.append(f"[amin, amax] = [{c[QC['amin']]}, {c[QC['amax']]}], the LUT's range is {list(want)}")
    accu = np.asarray(accu, np.float64)
    exdot = np.asarray(exdot, np.float64)
    amin, amax, exlo, exhi = (float(c[QC[k]]) for k in ("amin", "amax", "exlo", "exhi"))
    if accu.size and not (accu.min() >= amin and accu.max() <= amax):
        viol.append(f"accu range [{accu.min()}, {accu.max()}] outside [amin, amax] = [{amin}, {amax}]")
    if exdot.size and not (exdot.min() >= exlo and exdot.max() <= exhi):
        viol.append(f"ex-code dot range [{exdot.min()!r}, {exdot.max()!r}] outside [exlo, exhi] = [{exlo!r}, {exhi!r}]")
    q1 = float(np.abs(np.asarray(rq, np.float64)).sum())
    q1n = float(c[QC["q1norm"]])
    if not (q1 <= q1n <= q1 * Q1NORM_SLACK * (1 + 1e-4) + 1e-30):
        viol.append(f"q1norm {q1n!r} does not cover |q|_1 = {q1!r} within x{Q1NORM_SLACK}")
    return viol


def lut_range(lut8):
    """(amin, amax) of a u8 LUT [D/4][16]: the sums over codebooks of the smallest / largest entry."""
    t = np.asarray(lut8, np.int64).reshape(-1, 16)
    return int(t.min(1).sum()), int(t.max(1).sum())


def t_ub_rule(U, nvalid, top_k):
    """k_select_mfma's T_ub: the smallest finite U whose cumulative count of vectors in blocks with U' <= U reaches top_k
    (+inf when none does)."""
    U = np.asarray(U, F32)
    nvalid = np.asarray(nvalid, np.int64)
    best = F32(np.inf)
    for u in U[np.isfinite(U)]:
        if nvalid[U <= u].sum() >= top_k and u < best:
            best = u
    return best


def check_head_ub(cands, blocks, t_ub, top_k):
    """The lazy selection's head bounds.  cands: (gblock, U, nvalid) of every head candidate block as the kernel wrote them;
    blocks: gblock -> (dist, lb) arrays of that block's real vectors from the oracle; t_ub: the T_ub the kernel used (f32).
    U >= max(dist_v, lb_v) for every real vector, nvalid right, and T_ub == the rule's value over the tapped (U, nvalid)
    pairs bit for bit.  Returns (violations, stats: finite U count, candidates, median U / max(dist) over finite U)."""
    viol, ratios, nfin = [], [], 0
    for gb, U, nv in cands:
        U = F32(U)
        dist, lb = blocks[int(gb)]
        if nv != len(dist):
            viol.append(f"block {gb}: nvalid {nv}, has {len(dist)} real vectors")
            continue
        if not np.isfinite(U):
            if not U == np.inf:
                viol.append(f"block {gb}: U = {U!r}")
            continue
        nfin += 1
        with np.errstate(invalid="ignore"):
            top = np.fmax(dist.astype(np.float64), lb.astype(np.float64))
        if not (np.isfinite(top).all() and float(U) >= top.max()):
            i = int(np.nanargmax(top)) if np.isfinite(top).any() else 0
            viol.append(f"block {gb}: U = {U!r} < max(dist_v, lb_v) = {top[i]!r} (vector {i})")
            continue
        if top.max() > 0:
            ratios.append(float(U) / top.max())
    want = t_ub_rule([c[1] for c in cands], [c[2] for c in cands], top_k)
    if np.array([want], F32).view(np.uint32)[0] != np.array([t_ub], F32).view(np.uint32)[0]:
        viol.append(f"T_ub = {F32(t_ub)!r}, the rule over the tapped bounds gives {want!r}")
    return viol, {"finite": nfin, "cands": len(cands), "median_ratio": float(np.median(ratios)) if ratios else float("nan")}


def pack_sign_bits(bits, D):
    """The codes part of FastScan batch records [ceil(n/32) * D * 4] for sign bits [n][D], by the builder's own packers
    (pack_binary_code, then the 32-vector batch interleave)."""
    import rabitq_rs_amd as rq
    L = rq.builder.lib()
    n = bits.shape[0]
    rows = np.zeros((n, D // 8), np.uint8)
    for v in range(n):
        b = np.ascontiguousarray(bits[v], np.uint8)
        L.rbq_build_pack_binary_code(b.ctypes.data, rows[v].ctypes.data, D)
    packed = np.zeros(((n + 31) // 32) * 32 * (D // 8), np.uint8)
    L.rbq_build_pack_codes(rows.ctypes.data, n, D // 8, packed.ctypes.data)
    return packed


def extreme_bits(lut8, lowest):
    """[D] sign bits whose code takes, in every codebook, the nibble of the smallest (lowest) or largest LUT entry: the
    code's accu is then amin (or amax).  Nibble k of codebook j holds the bits of dims 4j..4j+3, most significant first."""
    t = np.asarray(lut8, np.int64).reshape(-1, 16)
    k = t.argmin(1) if lowest else t.argmax(1)
    return ((k[:, None] >> (3 - np.arange(4))) & 1).reshape(-1).astype(np.uint8)


class HostIndex:
    """An index described by numpy arrays in the reference's ClusterData layout, viewable by the oracle (the hdr_ptr /
    lists_ptr of builder.BuiltIndex) and writable as RBQ1 (rbq1_writer).  clusters: dicts with centroid, ids, batch_data,
    ex_codes [n][D * ex / 8], f_add_ex, f_rescale_ex, delta, vl."""

    def __init__(self, dim, padded_dim, metric, rotator, ex_bits, rotator_bytes, clusters):
        from rabitq_rs_amd._abi import Header, ListView
        self.clusters = []
        for c in clusters:
            n = len(c["ids"])
            self.clusters.append({
                "centroid": np.ascontiguousarray(c["centroid"], F32), "ids": np.ascontiguousarray(c["ids"], np.uint64),
                "batch_data": np.frombuffer(bytes(c["batch_data"]), np.uint8).copy(),
                "ex_codes": np.ascontiguousarray(np.asarray(c["ex_codes"], np.uint8).reshape(n, padded_dim * ex_bits // 8)),
                "f_add_ex": np.ascontiguousarray(c["f_add_ex"], F32), "f_rescale_ex": np.ascontiguousarray(c["f_rescale_ex"], F32),
                "delta": np.ascontiguousarray(c.get("delta", np.zeros(n)), F32), "vl": np.ascontiguousarray(c.get("vl", np.zeros(n)), F32)})
        self._rot = np.frombuffer(bytes(rotator_bytes) or b"\0", np.uint8).copy()
        self._hdr = Header(dim=dim, padded_dim=padded_dim, metric=metric, rotator=rotator, ex_bits=ex_bits, reserved=0,
                           n_vectors=sum(len(c["ids"]) for c in self.clusters), n_lists=len(self.clusters),
                           rotator_blob=self._rot.ctypes.data_as(C.POINTER(C.c_uint8)), rotator_len=len(rotator_bytes))
        self._lists = (ListView * max(len(self.clusters), 1))()
        for i, c in enumerate(self.clusters):
            lv = self._lists[i]
            lv.centroid = c["centroid"].ctypes.data_as(C.POINTER(C.c_float))
            lv.n = len(c["ids"])
            lv.ids = c["ids"].ctypes.data_as(C.POINTER(C.c_uint64))
            lv.batch_data = c["batch_data"].ctypes.data_as(C.POINTER(C.c_uint8))
            lv.batch_len = len(c["batch_data"])
            lv.ex_codes = c["ex_codes"].ctypes.data_as(C.POINTER(C.c_uint8)) if c["ex_codes"].size else None
            lv.f_add_ex = c["f_add_ex"].ctypes.data_as(C.POINTER(C.c_float))
            lv.f_rescale_ex = c["f_rescale_ex"].ctypes.data_as(C.POINTER(C.c_float))
        self.hdr_ptr = C.pointer(self._hdr)
        self.lists_ptr = C.cast(self._lists, C.POINTER(ListView))
        self.rotator_bytes = bytes(rotator_bytes)

    header = property(lambda self: self._hdr)
    padded_dim = property(lambda self: self._hdr.padded_dim)
    n_lists = property(lambda self: self._hdr.n_lists)

    def centroid(self, c):
        return self.clusters[c]["centroid"].copy()

    def list_sizes(self):
        return np.array([len(c["ids"]) for c in self.clusters], np.int64)

    def list_ids(self, c):
        return self.clusters[c]["ids"].copy()

    def list_arrays(self, c):
        return self.clusters[c]

    def rbq1(self):
        from rbq1_writer import write_rbq1
        h = self._hdr
        cl = [{**c, "ex_codes": [row.tobytes() for row in c["ex_codes"]], "batch_data": c["batch_data"].tobytes()}
              for c in self.clusters]
        return write_rbq1(int(h.dim), int(h.padded_dim), int(h.metric), int(h.rotator), int(h.ex_bits), self.rotator_bytes, cl)


def host_index_of(built):
    """A HostIndex holding copies of a builder.BuiltIndex's arrays (to be edited before it is written out)."""
    h = built.header
    return HostIndex(int(h.dim), int(h.padded_dim), int(h.metric), int(h.rotator), int(h.ex_bits), built.rotator_blob(),
                     [dict(built.list_arrays(c)) for c in range(int(h.n_lists))])
