"""An independent NumPy writer and parser of the crate's `.mstg` file (MstgIndex::save_main_index / load_main_index, reference
src/mstg/io.rs:129-245), written from io.rs and the struct definitions (MstgConfig src/mstg/config.rs:39-62, PostingList
src/mstg/posting_list.rs:7-32, RabitqConfig / QuantizedVector src/quantizer.rs:15-21, 63-88) under bincode 1.3's defaults.  It
shares no code with the library.  TEST INFRASTRUCTURE.

    "MSTG" | u32 1 | u64 77 | MstgConfig | u64 k | k x u32 ids | u64 k | k x (u64 len | PostingList) | u32 CRC-32 of bytes [8, here)
"""
import struct
import zlib

import numpy as np

CONFIG_FIELDS = ("max_posting_size", "branching_factor", "balance_weight", "closure_epsilon", "max_replicas", "rabitq_bits",
                 "faster_config", "metric", "hnsw_m", "hnsw_ef_construction", "centroid_precision", "default_ef_search",
                 "pruning_epsilon")
CONFIG_FMT = "<QQffQQBIQQIQf"
# MstgConfig::default()
DEFAULT_CONFIG = dict(max_posting_size=5000, branching_factor=10, balance_weight=1.0, closure_epsilon=0.15, max_replicas=8,
                      rabitq_bits=7, faster_config=False, metric=0, hnsw_m=32, hnsw_ef_construction=200, centroid_precision=1,
                      default_ef_search=150, pruning_epsilon=0.6)
FACTORS = ("delta", "vl", "f_add", "f_rescale", "f_error", "residual_norm", "f_add_ex", "f_rescale_ex")
KPERM0 = np.array([0, 8, 1, 9, 2, 10, 3, 11, 4, 12, 5, 13, 6, 14, 7, 15])


def config_bytes(cfg):
    return struct.pack(CONFIG_FMT, *(cfg[f] for f in CONFIG_FIELDS))


def ex_len(D, ex_bits):
    return D // 16 * {0: 2, 2: 4, 6: 12}[ex_bits]


def record_len(D, ex_bits):
    return 73 + 2 * D + D // 8 + ex_len(D, ex_bits)


def pack_ex(codes, ex_bits):
    """pack_ex_code_{2,6}bit_cpp_compat (src/simd.rs:2478-2541, 2601-2695) of codes [n][D]; ex_bits 0: D/16*2 zero bytes."""
    n, D = codes.shape
    c = codes.reshape(n, D // 16, 16).astype(np.uint32)
    if ex_bits == 0:
        return np.zeros((n, D // 16 * 2), np.uint8)
    two = lambda x: sum((x[:, :, 4 * g:4 * g + 4] & 3) << (2 * g) for g in range(4))  # noqa: E731 - byte m: codes 4g + m
    if ex_bits == 2:
        return two(c).astype(np.uint8).reshape(n, -1)
    lo = (c[:, :, :8] & 15) | ((c[:, :, 8:] & 15) << 4)
    return np.concatenate([lo, two(c >> 4)], axis=2).astype(np.uint8).reshape(n, -1)


def unpack_ex(packed, D, ex_bits):
    n = packed.shape[0]
    out = np.zeros((n, D // 16, 16), np.uint32)
    if ex_bits == 0:
        return out.reshape(n, D)
    p = packed.reshape(n, D // 16, 2 * ex_bits).astype(np.uint32)
    top = p if ex_bits == 2 else p[:, :, 8:]
    for g in range(4):
        out[:, :, 4 * g:4 * g + 4] = (top[:, :, :4] >> (2 * g)) & 3
    if ex_bits == 6:
        out <<= 4
        out[:, :, :8] |= p[:, :, :8] & 15
        out[:, :, 8:] |= p[:, :, :8] >> 4
    return out.reshape(n, D)


def lists_from_built(built, ids_of=None):
    """The posting lists of a builder.BuiltIndex (train_with_clusters over the expanded (vector, list) pairs, rotator NoRotation)
    as the writer's input: per list centroid, ids (mapped through ids_of), bits [n][D], ex [n][D] and the eight factors."""
    D, ex_bits = int(built.padded_dim), int(built.header.ex_bits)
    out = []
    for c in range(int(built.n_lists)):
        a = built.list_arrays(c)
        n = len(a["ids"])
        nb = (n + 31) // 32
        rec = a["batch_data"].reshape(nb, D * 4 + 384) if nb else np.zeros((0, D * 4 + 384), np.uint8)
        codes = rec[:, :D * 4].reshape(nb, D // 8, 32)
        # pack_codes (src/simd.rs:864-904): byte j (j' = j + 16) of a column holds the high (low) nibbles of vectors KPERM0[j] and + 16
        byte = np.zeros((nb, 32, D // 8), np.uint32)
        for j in range(16):
            v = KPERM0[j]
            hi, lo = codes[:, :, j].astype(np.uint32), codes[:, :, j + 16].astype(np.uint32)
            byte[:, v, :] = ((hi & 15) << 4) | (lo & 15)
            byte[:, v + 16, :] = ((hi >> 4) << 4) | (lo >> 4)
        bits = ((byte[..., None] >> (7 - np.arange(8))) & 1).reshape(nb * 32, D)[:n]
        fac = rec[:, D * 4:].copy().view(np.float32).reshape(nb, 3, 32)
        L = {"centroid": a["centroid"], "ids": a["ids"] if ids_of is None else np.asarray(ids_of)[a["ids"].astype(np.int64)].astype(np.uint64),
             "bits": bits.astype(np.uint32), "ex": unpack_ex(a["ex_codes"], D, ex_bits) if ex_bits else np.zeros((n, D), np.uint32),
             "delta": a["delta"], "vl": a["vl"], "residual_norm": built.list_residual_norm(c),
             "f_add_ex": a["f_add_ex"] if ex_bits else np.zeros(n, np.float32),
             "f_rescale_ex": a["f_rescale_ex"] if ex_bits else np.zeros(n, np.float32)}
        for i, name in enumerate(("f_add", "f_rescale", "f_error")):
            L[name] = fac[:, i, :].reshape(-1)[:n].copy()
        out.append(L)
    return out


def list_bytes(c, L, total_bits, t_const):
    """bincode of PostingList c.  An empty list carries RabitqConfig::default() (7, None): quantize_vectors returns before it
    sets the config."""
    D, n, ex_bits = len(L["centroid"]), len(L["ids"]), total_bits - 1
    tb, t = (total_bits, t_const) if n else (7, None)
    if "config" in L:  # a test's override
        tb, t = L["config"]
    head = struct.pack("<IQ", c, D) + np.asarray(L["centroid"], "<f4").tobytes() + struct.pack("<IQ", n, tb)
    head += b"\x00" if t is None else b"\x01" + np.float32(t).tobytes()
    head += struct.pack("<Q", n)
    if n == 0:
        return head
    E = ex_len(D, ex_bits)
    rec = np.zeros((n, record_len(D, ex_bits)), np.uint8)
    o = 0

    def put(a):
        nonlocal o
        a = np.ascontiguousarray(a).view(np.uint8).reshape(n, -1)
        rec[:, o:o + a.shape[1]] = a
        o += a.shape[1]
    u64 = lambda v: np.full(n, v, "<u8")  # noqa: E731
    put(np.asarray(L["ids"], "<u8"))
    put(u64(D)); put((L["ex"] + (L["bits"] << ex_bits)).astype("<u2"))
    put(u64(D // 8)); put(np.packbits(L["bits"].astype(np.uint8), axis=1, bitorder="big"))
    put(u64(E)); put(pack_ex(L["ex"], ex_bits))
    put(np.full(n, ex_bits, np.uint8)); put(u64(D))
    for f in FACTORS:
        put(np.asarray(L[f], "<f4"))
    assert o == rec.shape[1]
    return head + rec.tobytes()


def write(cfg, lists, t_const=None):
    """The whole stream.  cfg: dict of CONFIG_FIELDS; lists: as lists_from_built returns; t_const: None or the f32 of
    RabitqConfig::faster."""
    cb = config_bytes(cfg)
    body = struct.pack("<Q", len(cb)) + cb
    k = len(lists)
    body += struct.pack("<Q", k) + np.arange(k, dtype="<u4").tobytes() + struct.pack("<Q", k)
    parts = [body]
    for c, L in enumerate(lists):
        b = list_bytes(c, L, int(cfg["rabitq_bits"]), t_const)
        parts += [struct.pack("<Q", len(b)), b]
    body = b"".join(parts)
    return b"MSTG" + struct.pack("<I", 1) + body + struct.pack("<I", zlib.crc32(body))


def parse(data):
    """(cfg dict, lists, centroid ids, stored crc, (first, end) of the span the CRC covers).  Lists as the writer takes them,
    plus "config" = (total_bits, t_const or None), "code" [n][D] u16 as stored and the stream offsets "off" / "rec0"."""
    assert data[:4] == b"MSTG" and struct.unpack_from("<I", data, 4)[0] == 1
    o = 8
    (clen,) = struct.unpack_from("<Q", data, o); o += 8
    assert clen == struct.calcsize(CONFIG_FMT) == 77
    cfg = dict(zip(CONFIG_FIELDS, struct.unpack_from(CONFIG_FMT, data, o))); o += clen
    cfg["faster_config"] = bool(cfg["faster_config"])
    (k,) = struct.unpack_from("<Q", data, o); o += 8
    ids = np.frombuffer(data, "<u4", k, o).copy(); o += 4 * k
    (k2,) = struct.unpack_from("<Q", data, o); o += 8
    assert k2 == k
    ex_bits = cfg["rabitq_bits"] - 1
    lists = []
    for _ in range(k):
        off0 = o
        (ln,) = struct.unpack_from("<Q", data, o); o += 8
        end = o + ln
        cid, D = struct.unpack_from("<IQ", data, o); o += 12
        cent = np.frombuffer(data, "<f4", D, o).copy(); o += 4 * D
        size, tb, tag = struct.unpack_from("<IQB", data, o); o += 13
        t = None
        if tag:
            t = np.frombuffer(data, "<f4", 1, o)[0]; o += 4
        (n,) = struct.unpack_from("<Q", data, o); o += 8
        assert size == n
        R, E = record_len(D, ex_bits), ex_len(D, ex_bits)
        rec0 = o
        rec = np.frombuffer(data, np.uint8, n * R, o).reshape(n, R); o += n * R
        assert o == end
        p = 0

        def get(nbytes, dt):
            nonlocal p
            a = np.ascontiguousarray(rec[:, p:p + nbytes]).view(dt)
            p += nbytes
            return a
        L = {"cluster_id": cid, "centroid": cent, "config": (tb, t), "off": off0, "rec0": rec0}  # off: the length prefix; rec0: record 0
        L["ids"] = get(8, "<u8").reshape(-1)
        assert (get(8, "<u8") == D).all()
        L["code"] = get(2 * D, "<u2")
        assert (get(8, "<u8") == D // 8).all()
        L["bits"] = np.unpackbits(get(D // 8, np.uint8), axis=1, bitorder="big").astype(np.uint32).reshape(n, D)
        assert (get(8, "<u8") == E).all()
        L["ex"] = unpack_ex(get(E, np.uint8).reshape(n, E), D, ex_bits)
        assert (get(1, np.uint8) == ex_bits).all() and (get(8, "<u8") == D).all()
        for f in FACTORS:
            L[f] = get(4, "<f4").reshape(-1)
        assert p == R
        lists.append(L)
    (crc,) = struct.unpack_from("<I", data, o)
    assert o + 4 == len(data)
    return cfg, lists, ids, crc, (8, o)
