"""The `.mstg` format on the CPU (include/rbq_mstg_persist.h, csrc/host/rbq_mstg_file.hpp): the independent writer and parser of
tests/mstg_file.py against the library's framing and record validation, reached through the CPU builder's
rbq_build_mstg_file_check (the code rbq_mstg_load runs on the host, plus the CPU statement of the device's record checks)."""
import zlib

import numpy as np
import pytest

import mstg_file as mf
import mstg_persist_cases as pc
import rabitq_rs_amd as rq
from rabitq_rs_amd import _abi

# MstgConfig::default() under bincode 1.3: usize as u64, f32 bits, bool as u8, enum variants as u32 (L2 = 0, BF16 = 1)
DEFAULT_CONFIG_BYTES = bytes([
    0x88, 0x13, 0, 0, 0, 0, 0, 0,   # max_posting_size 5000
    10, 0, 0, 0, 0, 0, 0, 0,        # branching_factor
    0x00, 0x00, 0x80, 0x3f,         # balance_weight 1.0
    0x9a, 0x99, 0x19, 0x3e,         # closure_epsilon 0.15
    8, 0, 0, 0, 0, 0, 0, 0,         # max_replicas
    7, 0, 0, 0, 0, 0, 0, 0,         # rabitq_bits
    0,                              # faster_config false
    0, 0, 0, 0,                     # metric L2
    32, 0, 0, 0, 0, 0, 0, 0,        # hnsw_m
    200, 0, 0, 0, 0, 0, 0, 0,       # hnsw_ef_construction
    1, 0, 0, 0,                     # centroid_precision BF16
    150, 0, 0, 0, 0, 0, 0, 0,       # default_ef_search
    0x9a, 0x99, 0x19, 0x3f,         # pruning_epsilon 0.6
])


@pytest.fixture(scope="module")
def case():
    return pc.Case(D=16, bits=3, metric=0, faster=True)


def test_the_default_config_is_the_77_hand_listed_bytes():
    assert len(DEFAULT_CONFIG_BYTES) == 77
    assert mf.config_bytes(mf.DEFAULT_CONFIG) == DEFAULT_CONFIG_BYTES
    b = pc.tiny_file()
    assert b[16:16 + 77] == DEFAULT_CONFIG_BYTES[:32] + bytes([1]) + DEFAULT_CONFIG_BYTES[33:]  # (the tiny file is 1-bit)
    rc, detail, cfg, info = rq.builder.mstg_file_check(b)
    assert rc == _abi.RBQ_OK, detail
    assert cfg == dict(mf.DEFAULT_CONFIG, rabitq_bits=1, balance_weight=1.0, closure_epsilon=float(np.float32(0.15)),
                       pruning_epsilon=float(np.float32(0.6)))


@pytest.mark.parametrize("D,bits,metric,faster", [(16, 1, 0, True), (16, 3, 1, True), (48, 7, 0, False), (64, 7, 1, True)])
def test_writer_parses_back_and_the_library_accepts_it(D, bits, metric, faster):
    c = pc.Case(D, bits, metric, faster)
    b = c.bytes
    R = mf.record_len(D, bits - 1)
    assert R % 2 == 1 and R == {0: 109, 2: 111, 6: 119}[bits - 1] + (D - 16) * (2 + 1 / 8 + (bits - 1) / 8 + (1 / 8 if bits == 1 else 0))
    cfg, lists, ids, crc, (a, e) = mf.parse(b)
    assert crc == zlib.crc32(b[a:e]) and (a, e) == (8, len(b) - 4)
    assert np.array_equal(ids, np.arange(8))
    assert cfg["rabitq_bits"] == bits and cfg["metric"] == metric and cfg["faster_config"] == faster
    for i, (w, p) in enumerate(zip(c.lists, lists)):
        n = len(w["ids"])
        assert p["cluster_id"] == i and np.array_equal(p["centroid"], w["centroid"])
        want_t = None if c.t_const is None or n == 0 else c.t_const
        assert p["config"][0] == (bits if n else 7) and (p["config"][1] is None) == (want_t is None)
        for k in ("ids", "bits", "ex"):
            assert np.array_equal(p[k], w[k]), k
        assert np.array_equal(p["code"], w["ex"] + (w["bits"] << (bits - 1)))
        for f in mf.FACTORS:
            assert np.array_equal(p[f].view(np.uint32), np.asarray(w[f], np.float32).view(np.uint32)), f
    rc, detail, cfg2, info = rq.builder.mstg_file_check(b)
    assert rc == _abi.RBQ_OK, detail
    assert info == {"lists": 8, "vectors": len(c.pair_vec), "dim": D, "ex_bits": bits - 1}
    assert cfg2["rabitq_bits"] == bits and cfg2["max_posting_size"] == 80 and cfg2["default_ef_search"] == 6


def test_every_corruption_is_refused(case):
    assert rq.builder.mstg_file_check(case.bytes)[0] == _abi.RBQ_OK
    names = set()
    for name, bad, piece in pc.corruptions(case):
        rc, detail, _, _ = rq.builder.mstg_file_check(bad)
        assert rc == _abi.RBQ_INVALID_PERSISTENCE and detail and piece in detail, (name, rc, detail)
        names.add(name)
    assert len(names) >= 24


def test_one_bit_records_keep_nothing_in_their_unused_fields():
    b = bytearray(pc.tiny_file())
    _, L, _, _, _ = mf.parse(bytes(b))
    rec = L[0]["rec0"]
    for off in (16 + 32 + 8 + 2 + 8 + 1, 109 - 3):  # an ex byte; a byte of f_rescale_ex
        bad = bytearray(b)
        bad[rec + off] = 1
        rc, detail, _, _ = rq.builder.mstg_file_check(pc.fix_crc(bad))
        assert rc == _abi.RBQ_INVALID_PERSISTENCE and "1-bit" in detail, detail


def test_every_truncation_of_a_small_file_is_refused():
    b = pc.tiny_file()
    assert 400 < len(b) < 1000
    assert rq.builder.mstg_file_check(b)[0] == _abi.RBQ_OK
    for cut in pc.truncations(b):
        rc, detail, _, _ = rq.builder.mstg_file_check(cut)
        assert rc == _abi.RBQ_INVALID_PERSISTENCE and detail, (len(cut), rc, detail)
    for cut in pc.truncations(b, 7):  # the same with the last four bytes a valid checksum of what is left
        if len(cut) >= 12:
            rc, detail, _, _ = rq.builder.mstg_file_check(pc.fix_crc(cut))
            assert rc == _abi.RBQ_INVALID_PERSISTENCE and detail, (len(cut), rc, detail)


def test_residual_norm_of_the_builder_is_the_norm_of_the_residual(case):
    for c in (1, 4, 5):
        ids = case.built.list_ids(c).astype(np.int64)
        r = case.x[case.pair_vec[ids]].astype(np.float64) - case.c[c].astype(np.float64)
        want = np.sqrt((r * r).sum(axis=1))
        got = case.built.list_residual_norm(c)
        assert got.shape == want.shape and np.allclose(got, want, rtol=1e-5)
