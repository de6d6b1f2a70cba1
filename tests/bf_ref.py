"""CPU restatement of BruteForceRabitqIndex::search_internal (reference src/brute_force.rs:545-650), written from the crate
and not from the C++/HIP code: numpy sums vectorised over vectors but sequential over dimensions (float32 multiply, then add:
numpy does not fuse), the ex-code layouts of §A5, the oracle's rotation (ref_rotate) and the oracle's Rust-BinaryHeap
emulation (ref_heap_trace) for the top-k."""
import ctypes as C

import numpy as np

import oracle


def unpack_bits(bin_codes, D):
    """binary_code_packed [n][D/8] -> [n][D] {0,1}, MSB-first"""
    return np.unpackbits(bin_codes, axis=1, bitorder="big")[:, :D]


def unpack_ex(ex_codes, D, ex_bits):
    """ex_code_packed [n][D*ex/8] -> [n][D] codes (§A5: per 16 dimensions, 2-bit: one u32 word, code of dimension 4g+i at
    bits 8i+2g; 6-bit: 8 bytes of low nibbles — byte b holds dimension b (bits 0-3) and b+8 (bits 4-7) — then a u32 word of
    the top 2 bits laid out like the 2-bit code)"""
    n = ex_codes.shape[0]
    out = np.zeros((n, D), np.uint16)
    unit = 4 if ex_bits == 2 else 12
    for u in range(D // 16):
        blk = ex_codes[:, u * unit:(u + 1) * unit]
        w = blk[:, unit - 4:unit].copy().view("<u4")[:, 0].astype(np.uint32)
        for j in range(16):
            g, i = j >> 2, j & 3
            top = (w >> np.uint32(8 * i + 2 * g)) & np.uint32(3)
            if ex_bits == 2:
                out[:, u * 16 + j] = top
            else:
                byte = blk[:, j & 7].astype(np.uint32)
                lo = (byte >> np.uint32(0 if j < 8 else 4)) & np.uint32(15)
                out[:, u * 16 + j] = lo | (top << np.uint32(4))
    return out


def seq_dot(codes, rq):
    """sum_i (float)codes[:, i] * rq[i], sequential from +0.0f for every row"""
    acc = np.zeros(codes.shape[0], np.float32)
    for i in range(codes.shape[1]):
        acc = acc + codes[:, i].astype(np.float32) * np.float32(rq[i])
    return acc


def precompute(rq, ex_bits):
    """QueryPrecomputed::new (brute_force.rs:79-96)"""
    s = np.float32(0.0)
    for x in rq:
        s = np.float32(s + x)
    with np.errstate(all="ignore"):
        k1x = np.float32(np.float32(-0.5) * s)
        kbx = np.float32(np.float32(-(float(1 << ex_bits) - 0.5)) * s)
    return k1x, kbx, np.float32(1 << ex_bits)


class Prepared:
    """the index's arrays unpacked once (ids 0..n-1)"""

    def __init__(self, hdr_ptr, arrays):
        h = hdr_ptr.contents
        self.hdr_ptr, self.D, self.ex = hdr_ptr, int(h.padded_dim), int(h.ex_bits)
        self.metric = int(h.metric)
        self.bits = unpack_bits(arrays["bin"], self.D)
        self.codes = unpack_ex(arrays["ex"], self.D, self.ex) if self.ex else None
        self.a = arrays
        self.n = self.bits.shape[0]


def rotate(prep, q):
    x = np.ascontiguousarray(q, dtype=np.float32)
    out = np.empty(prep.D, np.float32)
    oracle.lib().ref_rotate(C.cast(prep.hdr_ptr, C.c_void_p), x.ctypes.data, out.ctypes.data)
    return out


def distances(prep, q):
    """every vector's distance for query q (float32 [n])"""
    rq = rotate(prep, q)
    k1x, kbx, bs = precompute(rq, prep.ex)
    with np.errstate(all="ignore"):
        bd = seq_dot(prep.bits, rq)
        if prep.ex == 0:
            return (prep.a["f_add"] + np.float32(0.0)) + prep.a["f_rescale"] * (bd + k1x)
        ed = seq_dot(prep.codes, rq)
        return (prep.a["f_add_ex"] + np.float32(0.0)) + prep.a["f_rescale_ex"] * (((bs * bd) + ed) + kbx)


def search(prep, q, top_k, allowed=None):
    """(ids u64, scores f32) of search_internal for one query; allowed = bool mask [n] or None"""
    d = distances(prep, q).astype(np.float32)
    keep = np.isfinite(d)
    if allowed is not None:
        keep &= allowed
    ids = np.nonzero(keep)[0].astype(np.uint64)
    dd = np.ascontiguousarray(d[keep], dtype=np.float32)
    out_ids = np.zeros(max(top_k, 1), np.uint64)
    out_d = np.zeros(max(top_k, 1), np.float32)
    n_out = C.c_uint32()
    rc = oracle.lib().ref_heap_trace(dd.ctypes.data, ids.ctypes.data, ids.size, top_k, out_ids.ctypes.data, out_d.ctypes.data,
                                     C.byref(n_out))
    assert rc == 0
    c = n_out.value
    # into_sorted_vec is ascending by total_cmp; the stable sorts that follow (L2: distance ascending, IP: score = -distance
    # descending) keep that order
    scores = out_d[:c] if prep.metric == 0 else -out_d[:c]
    return out_ids[:c], scores.astype(np.float32)


def scalar_search(prep, q, top_k):
    """plain-Python scalar loop of the whole search (tiny cases: self-check of the vectorised restatement)"""
    rq = rotate(prep, q)
    k1x, kbx, bs = precompute(rq, prep.ex)
    d = np.zeros(prep.n, np.float32)
    with np.errstate(all="ignore"):
        for v in range(prep.n):
            bd = np.float32(0.0)
            for i in range(prep.D):
                bd = np.float32(bd + np.float32(np.float32(prep.bits[v, i]) * rq[i]))
            if prep.ex == 0:
                d[v] = np.float32(np.float32(prep.a["f_add"][v] + np.float32(0)) + np.float32(prep.a["f_rescale"][v] * np.float32(bd + k1x)))
            else:
                ed = np.float32(0.0)
                for i in range(prep.D):
                    ed = np.float32(ed + np.float32(np.float32(prep.codes[v, i]) * rq[i]))
                t = np.float32(np.float32(np.float32(bs * bd) + ed) + kbx)
                d[v] = np.float32(np.float32(prep.a["f_add_ex"][v] + np.float32(0)) + np.float32(prep.a["f_rescale_ex"][v] * t))
    return d
