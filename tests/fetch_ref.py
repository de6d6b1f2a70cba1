"""A numpy restatement of the crate's `IvfRabitqIndex::fetch_embedding` (src/ivf.rs:1247-1307) over the bytes of an RBQ1-v3
stream (tests/rbq1_writer.py documents the layout), written from the algorithm: the FastScan sign bits (unpack_single_vector:
KPERM0 nibble pairing, MSB first), the cpp-compat ex codes (2 and 6 bits), code = ex + (bit << ex_bits), the rotated vector
(centroid + delta * code) + vl, then the rotator's inverse (inverse_rotate_into, src/rotation.rs:175-196 and 403-480).
TEST INFRASTRUCTURE.  Every float op is a float32 numpy op, one at a time and in the crate's order, so the results are the
crate's bit for bit (numpy vectorises only across independent elements)."""
import struct

import numpy as np

KPERM0 = np.array([0, 8, 1, 9, 2, 10, 3, 11, 4, 12, 5, 13, 6, 14, 7, 15])
F32 = np.float32


class Rbq1:
    """The parts of an RBQ1 stream fetch_embedding reads."""

    def __init__(self, data):
        o = 8
        (self.dim, self.padded_dim, self.metric, self.rotator, self.ex_bits, _total, _nv, nc, rot_len) = \
            struct.unpack_from("<IIBBBBQQQ", data, o)
        o += 36
        self.rot = bytes(data[o:o + rot_len])
        o += rot_len
        D = self.padded_dim
        self.clusters = []
        for _ in range(nc):
            cent = np.frombuffer(data, np.float32, D, o).copy(); o += 4 * D
            (n,) = struct.unpack_from("<Q", data, o); o += 8
            ids = np.frombuffer(data, np.uint64, n, o).copy(); o += 8 * n
            (blen,) = struct.unpack_from("<Q", data, o); o += 8
            batch = np.frombuffer(data, np.uint8, blen, o); o += blen
            exc = []
            for _ in range(n):
                (ln,) = struct.unpack_from("<Q", data, o); o += 8
                exc.append(np.frombuffer(data, np.uint8, ln, o)); o += ln
            o += 8 * n  # f_add_ex, f_rescale_ex
            delta = np.frombuffer(data, np.float32, n, o).copy(); o += 4 * n
            vl = np.frombuffer(data, np.float32, n, o).copy(); o += 4 * n
            self.clusters.append({"centroid": cent, "ids": ids, "batch": batch, "ex": exc, "delta": delta, "vl": vl})
        assert o + 4 == len(data), (o, len(data))


def sign_bits(batch, D, local):
    """unpack_single_vector: the padded_dim sign bits of vector `local` of a cluster (its FastScan batch record)."""
    rec = batch[(local // 32) * (D * 4 + 384):][:D * 4].reshape(D // 8, 32)
    v = local % 32
    j = int(np.nonzero(KPERM0 == v % 16)[0][0])  # KPERM0[j] = v % 16
    if v < 16:
        hi, lo = rec[:, j] & 15, rec[:, j + 16] & 15
    else:
        hi, lo = rec[:, j] >> 4, rec[:, j + 16] >> 4
    byte = (hi.astype(np.uint32) << 4) | lo
    return ((byte[:, None] >> (7 - np.arange(8))) & 1).reshape(-1).astype(np.uint32)


def ex_codes(packed, D, ex_bits):
    """unpack_ex_code for the cpp-compat packings (padded_dim % 16 == 0)."""
    if ex_bits == 0:
        return np.zeros(D, np.uint32)
    out = np.zeros(D, np.uint32)
    p = np.asarray(packed, np.uint8)
    if ex_bits == 2:
        w = p.reshape(D // 16, 4).astype(np.uint32)
        for i in range(4):  # byte i: bits 2g hold the code of dim 16t + 4g + i
            for g in range(4):
                out[4 * g + i::16] = (w[:, i] >> (2 * g)) & 3
        return out
    assert ex_bits == 6, ex_bits
    g12 = p.reshape(D // 16, 12).astype(np.uint32)
    for i in range(8):  # bytes 0-7: low nibbles of dims i (low half) and i + 8 (high half)
        out[i::16] = g12[:, i] & 15
        out[i + 8::16] = g12[:, i] >> 4
    for i in range(4):  # bytes 8-11: the top two bits, laid out like the 2-bit packing
        for g in range(4):
            out[4 * g + i::16] |= ((g12[:, 8 + i] >> (2 * g)) & 3) << 4
    return out


def rotated(idx, c, local):
    """fetch_embedding steps 1-3: the reconstruction in rotated space of vector `local` of cluster c."""
    cl, D, ex = idx.clusters[c], idx.padded_dim, idx.ex_bits
    code = ex_codes(cl["ex"][local], D, ex) + (sign_bits(cl["batch"], D, local) << ex)
    t = cl["centroid"] + cl["delta"][local] * code.astype(F32)
    return (t + cl["vl"][local]).astype(F32)


def _fht(x):
    """fht over the last axis (a power of two long): stage h pairs (j, j + h)."""
    B, n = x.shape
    h = 1
    while h < n:
        y = x.reshape(B, n // (2 * h), 2, h)
        a, b = y[:, :, 0, :], y[:, :, 1, :]
        x = np.stack([a + b, a - b], axis=2).reshape(B, n)
        h *= 2
    return x


def _flip(x, bits):
    return np.where(bits[None, :] != 0, -x, x)


def inverse_rotate(dim, padded_dim, rotator, rot, rows):
    """inverse_rotate_into of every row of `rows` [B][padded_dim] f32 -> [B][dim]."""
    D = padded_dim
    x = np.array(rows, dtype=F32).reshape(-1, D)
    if rotator == 0:  # Matrix: out[col] = sum_row R[row][col] * rotated[row], serially from 0.0
        R = np.frombuffer(rot, np.float32).reshape(D, D)
        acc = np.zeros((x.shape[0], dim), F32)
        for r in range(D):
            acc = acc + R[r, :dim][None, :] * x[:, r:r + 1]
        return acc
    assert rotator == 1, rotator
    trunc = 1 << (int(dim).bit_length() - 1)
    fac = F32(1.0) / np.sqrt(F32(trunc))
    rfac, rlen = F32(1.0) / fac, F32(1.0) / F32(trunc)
    fo = D // 8
    flips = [np.unpackbits(np.frombuffer(rot, np.uint8)[r * fo:(r + 1) * fo], bitorder="little")[:D] for r in range(4)]
    if trunc == D:
        for r in (3, 2, 1, 0):
            x = x * rfac
            x = _fht(x)
            x = x * rlen
            x = _flip(x, flips[r])
    else:
        start, half = D - trunc, D // 2
        x = x * F32(4.0)
        for r in (3, 2, 1, 0):
            x = x * F32(0.5)
            a, b = x[:, :half], x[:, half:]
            x = np.concatenate([a + b, a - b], axis=1)
            seg = slice(start, D) if r & 1 else slice(0, trunc)
            s = x[:, seg] * rfac
            s = _fht(s)
            x[:, seg] = s * rlen
            x = _flip(x, flips[r])
    return np.ascontiguousarray(x[:, :dim], dtype=F32)


def fetch(data, ids):
    """fetch_embedding of every id of `ids` over the RBQ1 stream `data`: (out [n][dim] f32, found [n] bool).  The first
    occurrence in (cluster, position) order wins; a missing id gives a zero row and False."""
    idx = data if isinstance(data, Rbq1) else Rbq1(data)
    where = {}
    for c, cl in enumerate(idx.clusters):
        for p, i in enumerate(cl["ids"].tolist()):
            where.setdefault(int(i), (c, p))
    ids = [int(i) for i in np.asarray(ids, np.uint64).reshape(-1)]
    uniq = sorted({i for i in ids if i in where})
    rows = np.stack([rotated(idx, *where[i]) for i in uniq]) if uniq else np.zeros((0, idx.padded_dim), F32)
    vecs = inverse_rotate(idx.dim, idx.padded_dim, idx.rotator, idx.rot, rows)
    pos = {i: k for k, i in enumerate(uniq)}
    out = np.zeros((len(ids), idx.dim), F32)
    found = np.zeros(len(ids), bool)
    for k, i in enumerate(ids):
        if i in pos:
            out[k] = vecs[pos[i]]
            found[k] = True
    return out, found


def all_ids(data):
    """Every id of the stream in (cluster, position) order."""
    idx = data if isinstance(data, Rbq1) else Rbq1(data)
    return np.concatenate([cl["ids"] for cl in idx.clusters]) if idx.clusters else np.zeros(0, np.uint64)
