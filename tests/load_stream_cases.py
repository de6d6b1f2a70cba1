"""The error corpus of the streamed RBQ1 loader (rbq_index_load_rbq1_stream), shared by tests/test_gpu_load_stream.py (both
loaders on the GPU) and tests/test_load_stream_host.py (the GPU-free half against rbq1_parse under ASan + UBSan).  TEST
INFRASTRUCTURE.  Every case is (name, bytes); what the right answer is, is never stated here: the whole-buffer loader says."""
import struct
import zlib

import numpy as np

import rbq1_writer

SIZES = [3, 33, 0, 5]   # list 0: a few vectors; list 1: one past a block; list 2: empty; list 3: short
DIM = 64                 # FhtKac: padded_dim 64, 32 rotator bytes
EX_BITS = 6
EXB = DIM * EX_BITS // 8
STRIDE = DIM * 4 + 384
CLUSTER0 = 44 + DIM // 2


def base_stream():
    """a dim-64, 7-bit, 4-list stream of a few KB from the CPU builder"""
    import rabitq_rs_amd as rq
    from conftest import make_dataset
    rng = np.random.default_rng(5)
    data = make_dataset(sum(SIZES), DIM, 3, 11)
    assign = rng.permutation(np.repeat(np.arange(len(SIZES)), SIZES)).astype(np.uint32)
    cent = np.stack([data[assign == c].mean(0) if s else data[c] for c, s in enumerate(SIZES)]).astype(np.float32)
    built = rq.builder.train_with_clusters(data, cent, assign, EX_BITS + 1, 0, 1, 21, True)
    out = built.save_rbq1()
    built.close()
    return bytes(out)


def layout(sizes=SIZES, d=DIM, exb=EXB, cluster0=CLUSTER0):
    """per list: dict of the file offsets of its fields (ex: one offset per vector, of the length prefix)"""
    out, off = [], cluster0
    for n in sizes:
        nb = (n + 31) // 32
        L = {"start": off, "n": off + d * 4}
        L["ids"] = L["n"] + 8
        L["blen"] = L["ids"] + n * 8
        L["batch"] = L["blen"] + 8
        L["ex"] = [L["batch"] + nb * (d * 4 + 384) + v * (8 + exb) for v in range(n)]
        L["fadd"] = L["batch"] + nb * (d * 4 + 384) + n * (8 + exb)
        L["fres"], L["delta"], L["vl"] = L["fadd"] + 4 * n, L["fadd"] + 8 * n, L["fadd"] + 12 * n
        L["end"] = L["fadd"] + 16 * n
        out.append(L)
        off = L["end"]
    return out, off  # (lists, offset of the stored CRC)


def _patch(s, off, fmt, value, fix_crc=False):
    b = bytearray(s)
    struct.pack_into(fmt, b, off, value)
    if fix_crc:
        _, crc_off = layout()
        struct.pack_into("<I", b, crc_off, zlib.crc32(bytes(b[8:crc_off])) & 0xFFFFFFFF)
    return bytes(b)


def _flip(s, off, bit=0):
    b = bytearray(s)
    b[off] ^= 1 << bit
    return bytes(b)


def _random_stream(ex_bits, sizes, d=DIM, seed=3):
    """a self-consistent stream of random bytes from the independent writer (any ex_bits the format allows)"""
    rng = np.random.default_rng(seed)
    exb = d * ex_bits // 8
    clusters = []
    for n in sizes:
        nb = (n + 31) // 32
        f = lambda k: [float(x) for x in rng.standard_normal(k).astype(np.float32)]  # noqa: E731
        clusters.append({"centroid": f(d), "ids": [int(x) for x in rng.integers(0, 1 << 40, n)],
                         "batch_data": rng.integers(0, 256, nb * (d * 4 + 384), dtype=np.uint8).tobytes(),
                         "ex_codes": [rng.integers(0, 256, exb, dtype=np.uint8).tobytes() for _ in range(n)],
                         "f_add_ex": f(n), "f_rescale_ex": f(n), "delta": f(n), "vl": f(n)})
    return rbq1_writer.write_rbq1(d, d, 0, 1, ex_bits, rng.integers(0, 256, d // 2, dtype=np.uint8).tobytes(), clusters)


def header_cases(s):
    lists, crc_off = layout()
    L1 = lists[1]
    c = [("good", s)]
    c.append(("wrong magic", b"RBQ2" + s[4:]))
    c.append(("wrong version", _patch(s, 4, "<I", 2)))
    c.append(("dim 0", _patch(s, 8, "<I", 0)))
    c.append(("padded_dim < dim", _patch(s, 12, "<I", DIM - 16)))
    c.append(("metric tag", _patch(s, 16, "<B", 2)))
    c.append(("rotator tag", _patch(s, 17, "<B", 2)))
    c.append(("ex_bits tag 17", _patch(_patch(s, 18, "<B", 17), 19, "<B", 18)))
    c.append(("total_bits 0", _patch(s, 19, "<B", 0)))
    c.append(("total_bits 17", _patch(s, 19, "<B", 17)))
    c.append(("total_bits != ex_bits + 1", _patch(s, 19, "<B", EX_BITS + 2)))
    c.append(("rotator length + 4", _patch(s, 36, "<Q", DIM // 2 + 4)))
    c.append(("rotator length - 4", _patch(s, 36, "<Q", DIM // 2 - 4)))
    c.append(("rotator length past the end", _patch(s, 36, "<Q", len(s))))
    c.append(("ex_bits 4 in the header only", _patch(_patch(s, 18, "<B", 4), 19, "<B", 5)))
    c.append(("ex_bits 4, consistent stream", _random_stream(4, SIZES)))
    c.append(("ex_bits 1, consistent stream", _random_stream(1, [2, 0, 40])))
    c.append(("padded_dim 48 under FhtKac, consistent stream", _random_stream(2, [1, 33], d=48)))
    c.append(("no clusters", _random_stream(6, [])))
    c.append(("cluster_count huge", _patch(s, 28, "<Q", 1 << 40)))
    c.append(("cluster_count + 1", _patch(s, 28, "<Q", len(SIZES) + 1)))
    c.append(("cluster_count - 1", _patch(s, 28, "<Q", len(SIZES) - 1)))
    c.append(("cluster n 1000001", _patch(s, L1["n"], "<Q", 1000001)))
    c.append(("cluster n + 1", _patch(s, L1["n"], "<Q", SIZES[1] + 1)))
    c.append(("batch_data length + 1", _patch(s, L1["blen"], "<Q", 2 * STRIDE + 1)))
    c.append(("batch_data length one record short", _patch(s, L1["blen"], "<Q", STRIDE)))
    for v, where in ((0, "first"), (16, "middle"), (32, "last")):
        c.append((f"ex prefix of the {where} vector", _patch(s, L1["ex"][v], "<Q", EXB + 1)))
        c.append((f"ex prefix of the {where} vector, high word", _patch(s, L1["ex"][v] + 4, "<I", 1)))
    c.append(("ex prefix of list 0", _patch(s, lists[0]["ex"][1], "<Q", 0)))
    c.append(("ex prefix of the last list", _patch(s, lists[3]["ex"][4], "<Q", EXB - 1)))
    c.append(("vector_count + 1", _patch(s, 20, "<Q", sum(SIZES) + 1)))
    c.append(("vector_count - 1", _patch(s, 20, "<Q", sum(SIZES) - 1)))
    c.append(("bit flip in ids", _flip(s, L1["ids"] + 21, 3)))
    c.append(("bit flip in batch_data", _flip(s, L1["batch"] + STRIDE + 7, 6)))
    c.append(("bit flip in an ex code", _flip(s, L1["ex"][5] + 8 + 11, 1)))
    c.append(("bit flip in a centroid", _flip(s, lists[2]["start"] + 9, 0)))
    c.append(("bit flip in the rotator", _flip(s, 50, 2)))
    c.append(("bit flip in the header's vector count, CRC refreshed", _patch(s, 20, "<Q", sum(SIZES) ^ 4, fix_crc=True)))
    c.append(("stored CRC flipped", _flip(s, crc_off + 2, 5)))
    c.append(("junk after the CRC", s + bytes(range(200)) * 5))
    return c


def truncation_cases(s):
    lists, crc_off = layout()
    cuts = {0, 4, 8, 12, 16, 20, 28, 36, 44, CLUSTER0, crc_off, crc_off + 4}
    for L, vs in ((lists[0], (0, 1, 2)), (lists[1], (0, 1, 16, 32))):
        cuts |= {L[k] for k in ("start", "n", "ids", "blen", "batch", "fadd", "fres", "delta", "vl", "end")}
        for v in vs:
            cuts |= {L["ex"][v], L["ex"][v] + 8}
    offs = set()
    for c in cuts:
        offs |= {c - 1, c, c + 1}
    offs |= set(range(0, len(s), 97))
    return [(f"cut at {o}", s[:o]) for o in sorted(o for o in offs if 0 <= o < len(s))]


def order_cases(s):
    lists, crc_off = layout()
    L1, L2, L3 = lists[1], lists[2], lists[3]
    bad_prefix = lambda b, L, v: _patch(b, L["ex"][v], "<Q", EXB + 7)  # noqa: E731
    c = []
    c.append(("prefix in list 1 + batch_data length in list 2", _patch(bad_prefix(s, L1, 20), L2["blen"], "<Q", 1)))
    c.append(("prefix + batch_data length, both in list 1", _patch(bad_prefix(s, L1, 20), L1["blen"], "<Q", STRIDE)))
    c.append(("prefix in list 1 + bit flip in list 3", _flip(bad_prefix(s, L1, 32), L3["ids"] + 3)))
    c.append(("prefix in list 3 + batch_data length in list 1", _patch(bad_prefix(s, L3, 0), L1["blen"], "<Q", STRIDE)))
    c.append(("prefix in list 3 + cluster n of list 2 too large", _patch(bad_prefix(s, L3, 0), L2["n"], "<Q", 1 << 33)))
    c.append(("prefix in list 1 + cluster n of list 3 too large", _patch(bad_prefix(s, L1, 0), L3["n"], "<Q", 1 << 33)))
    c.append(("prefix in list 1 + cut inside list 3", bad_prefix(s, L1, 7)[:L3["ex"][2] + 3]))
    c.append(("prefix in list 3 behind the cut", bad_prefix(s, L3, 3)[:L3["ex"][2] + 3]))
    c.append(("cut inside the code of a wrong prefix", bad_prefix(s, L3, 2)[:L3["ex"][2] + 20]))
    c.append(("cut inside a wrong prefix", bad_prefix(s, L3, 2)[:L3["ex"][2] + 5]))
    c.append(("prefix in list 1 + vector_count + 1", _patch(bad_prefix(s, L1, 1), 20, "<Q", sum(SIZES) + 1)))
    c.append(("vector_count + 1 + stored CRC cut off", _patch(s, 20, "<Q", sum(SIZES) + 1)[:crc_off + 2]))
    c.append(("bit flip + stored CRC cut off", _flip(s, L1["ids"] + 2)[:crc_off + 3]))
    return c


def corpus(s):
    return header_cases(s) + truncation_cases(s) + order_cases(s)
