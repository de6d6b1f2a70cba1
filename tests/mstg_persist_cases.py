"""Shared inputs of the `.mstg` persistence tests (tests/test_mstg_persist_host.py, tests/test_gpu_mstg_persist.py): small MSTG
indexes with hand-placed centroids, their files from the independent writer (tests/mstg_file.py) over the CPU builder's arrays,
and the corruptions a loader must refuse.  TEST INFRASTRUCTURE."""
import struct
import zlib

import numpy as np

import mstg_file as mf
import rabitq_rs_amd as rq
from rabitq_rs_amd import mstg

SIZES = (1, 31, 32, 33, 65)  # the lists the hand-placed centroids pin: below, at and above one and two 32-vector blocks
EPS, REPLICAS = 0.15, 4


def points(D, seed=0):
    """About 300 vectors and 8 centroids: lists 0-4 hold exactly SIZES (far apart: one list per vector), lists 5 and 6 lie on
    either side of their vectors (most of which sit in both), list 7 is far from everything and receives none."""
    rng = np.random.default_rng(seed)
    k = 8
    c = np.zeros((k, D), np.float32)
    for i in range(5):
        c[i, i % D] = 100.0 * (i + 1)
        c[i, (i + 5) % D] = -50.0 * (i + 1)
    c[5, :] = 1.0
    c[6, :] = -1.0
    c[7, :] = -1000.0
    rows = [c[i] + 0.5 * rng.standard_normal((n, D)) for i, n in enumerate(SIZES)]
    rows.append(0.5 * (c[5] + c[6]) + 0.3 * rng.standard_normal((138, D)))
    x = np.concatenate(rows).astype(np.float32)
    return x[rng.permutation(len(x))].copy(), c


class Case:
    """One index on the CPU: the closure, the builder's arrays over the expanded pairs, the writer's lists and bytes."""

    def __init__(self, D=16, bits=3, metric=0, faster=True, seed=0):
        self.D, self.bits, self.metric, self.faster = D, bits, metric, faster
        self.x, self.c = points(D, seed)
        lists, counts = rq.closure_assign_cpu(self.x, self.c, EPS, REPLICAS)
        self.pair_vec, self.pair_list = mstg.expand_pairs(lists, counts)
        self.built = rq.builder.train_with_clusters(self.x[self.pair_vec], self.c, self.pair_list, bits, metric,
                                                    rq.RotatorType.NoRotation, 42, faster)
        sizes = self.built.list_sizes()
        assert tuple(sizes[:5]) == SIZES and sizes[7] == 0 and sizes[5] + sizes[6] > 160, sizes
        self.t_const = np.float32(self.built.t_const) if faster and bits > 1 else None
        self.cfg = dict(mf.DEFAULT_CONFIG, rabitq_bits=bits, faster_config=faster, metric=metric, max_posting_size=80,
                        max_replicas=REPLICAS, closure_epsilon=EPS, hnsw_ef_construction=400, default_ef_search=6)
        self.lists = mf.lists_from_built(self.built, self.pair_vec)
        self.bytes = mf.write(self.cfg, self.lists, self.t_const)


def tiny_file():
    """Three lists of 2, 0 and 1 vectors at D = 16, 1 bit: a file of a few hundred bytes whose every prefix is tried."""
    rng = np.random.default_rng(3)
    lists = []
    for n in (2, 0, 1):
        L = {"centroid": rng.standard_normal(16).astype(np.float32), "ids": np.arange(n, dtype=np.uint64) + 10,
             "bits": rng.integers(0, 2, (n, 16)).astype(np.uint32), "ex": np.zeros((n, 16), np.uint32)}
        for f in mf.FACTORS:
            L[f] = rng.standard_normal(n).astype(np.float32)
        L["f_add_ex"][:] = 0
        L["f_rescale_ex"][:] = 0
        lists.append(L)
    return mf.write(dict(mf.DEFAULT_CONFIG, rabitq_bits=1), lists, None)


def fix_crc(b):
    b = bytearray(b)
    b[-4:] = struct.pack("<I", zlib.crc32(bytes(b[8:-4])))
    return bytes(b)


def corruptions(case):
    """(name, bytes, a piece of the loader's message) for every refusal of the loader's list, one case each.  Unless the case
    is the checksum itself the CRC is made valid again, so the loader goes past it.  `case`: a 3-bit faster-config Case."""
    assert case.bits == 3 and case.faster
    good = case.bytes
    _, L, _, _, _ = mf.parse(good)
    D = case.D
    R = mf.record_len(D, 2)
    o_bin, o_ex = 16 + 2 * D, 16 + 2 * D + 8 + D // 8
    o_tail = o_ex + 8 + mf.ex_len(D, 2)
    hdr = lambda c: L[c]["off"] + 8  # noqa: E731 - cluster_id of list c; centroid length at + 4
    cfg_at = 8 + 8
    ids_at = cfg_at + 77 + 8

    def put(off, raw, crc=True):
        b = bytearray(good)
        b[off:off + len(raw)] = raw
        return fix_crc(b) if crc else bytes(b)
    u64, u32 = (lambda v: struct.pack("<Q", v)), (lambda v: struct.pack("<I", v))  # noqa: E731
    rec1 = L[1]["rec0"] + 3 * R  # a record of the 31-vector list
    size_at = hdr(2) + 12 + 4 * D
    out = [
        ("magic", put(0, b"MSTX"), "invalid magic"),
        ("version", put(4, u32(2)), "unsupported version"),
        ("crc", put(rec1 + o_tail + 9 + 8, b"\x55", crc=False), "checksum mismatch"),
        ("config length", put(8, u64(78)), "77 bytes"),
        ("length past the stream", put(L[0]["off"], u64(1 << 40)), "ends early"),
        ("list count past the stream", put(ids_at - 8, u64(1 << 50)), "ends early"),
        ("dim % 16", put(hdr(0) + 4, u64(24)), "multiple of 16"),
        ("ex_bits outside {0, 2, 6}", put(cfg_at + 32, u64(5)), "rabitq_bits must be"),
        ("metric variant", put(cfg_at + 41, u32(2)), "metric"),
        ("list bits differ from the config", put(size_at + 4, u64(7)), "total_bits differs"),
        ("t_const differs between lists", put(size_at + 13, np.float32(case.t_const * 2).tobytes()), "t_const differ"),
        ("t_const tag", put(size_at + 12, b"\x02"), "Option tag"),
        ("size != vectors.len()", put(size_at, u32(33)), "size differs"),
        ("list length is not header + records", put(L[3]["off"], u64(struct.unpack_from("<Q", good, L[3]["off"])[0] - 1)), ""),
        ("centroid ids out of order", put(ids_at, u32(1) + u32(0)), "centroid ids"),
        ("cluster ids out of order", put(hdr(1), u32(0)), "cluster ids"),
        ("centroid lengths differ", put(hdr(2) + 4, u64(32)), ""),
        ("empty list with another config", put(hdr(7) + 12 + 4 * D + 4, u64(3)), "empty posting list"),
        ("record: code length", put(rec1 + 8, u64(D + 1)), "code length"),
        ("record: binary length", put(rec1 + o_bin, u64(D // 8 + 1)), "binary_code_packed length"),
        ("record: ex length", put(rec1 + o_ex, u64(0)), "ex_code_packed length"),
        ("record: ex_bits", put(rec1 + o_tail, b"\x06"), "ex_bits"),
        ("record: dim", put(rec1 + o_tail + 1, u64(D + 16)), "dim"),
        ("record: code is not ex + (bit << ex_bits)", put(rec1 + 16 + 2 * 5, bytes([good[rec1 + 16 + 2 * 5] ^ 1])), "code is not"),
    ]
    b = bytearray(good)
    b[-4:-4] = b"\x00" * 5
    out.append(("bytes before the checksum", fix_crc(b), ""))
    out.append(("bytes after the checksum", good + b"\x00", ""))
    return out


def truncations(b, step=1):
    return [b[:n] for n in range(0, len(b), step)]
