"""Dimension edges without a GPU: the oracle's FhtKacRotator::rotate (the yardstick of every GPU comparison in
tests/test_gpu_dim_edges.py) against a float64 restatement of src/rotation.rs:350-401 at trunc 1-8, odd dims and D = 2048; and the
refusals of dim 2049 (padded_dim 2112: the crate's high-accuracy i32 LUT mode, which this build does not serve) and of a Matrix
dim that is not a multiple of 16 by the RBQ1 / RBF1 readers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fetch_ref
import oracle
import rabitq_rs_amd as rq
from conftest import ROOT, build_index, make_dataset
from rabitq_rs_amd import bruteforce as bfm
from rabitq_rs_amd import index as ix
from rbf1_writer import FACTORS, write_rbf1
from rbq1_writer import from_built, write_rbq1

# one dimension table for the host and the GPU file: trunc 1/2/4/8 padded to 64; odd dims around multiples of 64; D = 2048 on the
# Kac path (trunc 1024) and as a power of two (rotate_fhtkac_wave<32>)
KAC_DIMS = [1, 2, 3, 5, 7, 8, 9, 15, 17, 31, 33, 63, 65, 127, 129, 255, 257, 513, 1023, 1025, 1985, 2000, 2047, 2048]
MATRIX_DIMS = [16, 80, 1008, 2048]
P, CFG = rq._abi.RBQ_INVALID_PERSISTENCE, rq._abi.RBQ_INVALID_CONFIG
TOO_WIDE = "padded_dim > 2048 (high-accuracy i32 LUT mode) is not supported"
NOT_16 = "Dimension must be multiple of 16 for SIMD"


def rotate_f64(dim, D, flip_bytes, x):
    """FhtKacRotator::rotate_into in float64: zero-pad to D; trunc == D: 4 x (flip, fht, * fac); else 4 x (flip, fht of the head
    (rounds 1, 3) or the tail (rounds 2, 4) of length trunc, * fac on it, Kac's walk), then * 0.25."""
    trunc = 1 << (int(dim).bit_length() - 1)
    fac = 1.0 / np.sqrt(float(trunc))
    fo = D // 8
    flips = [np.unpackbits(np.frombuffer(flip_bytes, np.uint8)[r * fo:(r + 1) * fo], bitorder="little")[:D] for r in range(4)]
    v = np.zeros((1, D), np.float64)
    v[0, :dim] = np.asarray(x, np.float64)
    if trunc == D:
        for r in range(4):
            v = fetch_ref._fht(fetch_ref._flip(v, flips[r])) * fac
        return v[0]
    start, half = D - trunc, D // 2
    for r in range(4):
        v = fetch_ref._flip(v, flips[r])
        seg = slice(0, trunc) if r % 2 == 0 else slice(start, D)
        v[:, seg] = fetch_ref._fht(v[:, seg]) * fac
        v = np.concatenate([v[:, :half] + v[:, half:], v[:, :half] - v[:, half:]], axis=1)
    return v[0] * 0.25


@pytest.mark.parametrize("dim", KAC_DIMS)
def test_oracle_rotation_matches_float64_restatement(dim):
    """f32 oracle against the f64 statement: within a few f32 ulps of ||x|| per coordinate (each output is a +-1 combination over
    log2(trunc) + 4 levels, every level rounded once), norm preserved, and fetch_ref's inverse brings x back."""
    _, built = build_index(n=8, dim=dim, nlist=1, total_bits=7, seed=900 + dim)
    D = built.padded_dim
    assert D == (dim + 63) // 64 * 64 and built.hdr.rotator == 1
    blob = built.rotator_blob()
    assert len(blob) == 4 * D // 8
    rng = np.random.default_rng(dim)
    xs = [rng.standard_normal(dim).astype(np.float32), (rng.random(dim) * 100).astype(np.float32),
          np.eye(dim, dtype=np.float32)[dim - 1], np.full(dim, -3.0, np.float32)]
    levels = int(np.log2(1 << (dim.bit_length() - 1))) + 8
    for x in xs:
        got = oracle.rotate(built, x)
        assert got.shape == (D,) and got.dtype == np.float32
        want = rotate_f64(dim, D, blob, x)
        nx = float(np.linalg.norm(x.astype(np.float64)))
        err = np.abs(got.astype(np.float64) - want).max()
        assert err <= 4 * levels * np.finfo(np.float32).eps * nx, (dim, err, nx)
        assert abs(np.linalg.norm(got.astype(np.float64)) - nx) <= 1e-5 * nx, dim
        back = fetch_ref.inverse_rotate(dim, D, 1, blob, got[None, :])[0]
        np.testing.assert_allclose(back, x, rtol=0, atol=8 * levels * np.finfo(np.float32).eps * nx)
        # the builder's own rotation (the encoder's) is the oracle's, bit for bit
        assert np.array_equal(built.rotate(x).view(np.uint32), got.view(np.uint32))


def test_restatement_is_not_trivially_satisfied():
    """the f64 restatement sees a wrong flip table, a wrong trunc and a missing closing scale (so the test above can fail)"""
    _, built = build_index(n=8, dim=33, nlist=1, total_bits=7, seed=7)
    x = make_dataset(1, 33, 1, 8)[0]
    blob = bytearray(built.rotator_blob())
    good = rotate_f64(33, 64, bytes(blob), x)
    assert np.abs(good - oracle.rotate(built, x)).max() < 1e-5
    blob[3] ^= 0x10
    assert np.abs(rotate_f64(33, 64, bytes(blob), x) - good).max() > 1e-3
    assert np.abs(rotate_f64(64, 64, built.rotator_blob(), np.r_[x, np.zeros(31, np.float32)]) - good).max() > 1e-3  # trunc 64


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _load_rbq1(blob):
    h = C.c_void_p()
    buf = (C.c_uint8 * len(blob)).from_buffer_copy(bytes(blob))
    rc = ix.lib().rbq_index_load_rbq1(buf, len(blob), 1, None, C.byref(h))
    return rc, h.value, ix._detail()


def _load_rbf1(blob):
    h = C.c_void_p()
    buf = (C.c_uint8 * len(blob)).from_buffer_copy(bytes(blob))
    rc = bfm.lib().rbq_bf_load_rbf1(buf, len(blob), -1, C.byref(h))
    return rc, h.value, ix._detail()


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostcheck_dims") / "librbq_hostcheck.so")
    subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-O1", "-I", os.path.join(ROOT, "include"), "-shared", "-o", out,
                           os.path.join(ROOT, "rabitq-rs_amd", "csrc", "host", "rbq_hostcheck.cpp")])
    L = C.CDLL(out)
    for f in (L.rbq_hostcheck_parse, L.rbq_hostcheck_parse_rbf1):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def _hostcheck(fn, blob):
    buf = (C.c_uint8 * len(blob)).from_buffer_copy(bytes(blob))
    det = C.create_string_buffer(256)
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = fn(buf, len(blob), det, 256, C.byref(a), C.byref(b), C.byref(c))
    return rc, det.value.decode()


@pytest.mark.parametrize("metric,bits", [(0, 7), (1, 3), (0, 1)])
def test_rbq1_of_dim_2049_is_refused(hostcheck, metric, bits):
    """The CPU builder builds dim 2049 as the crate does (padded_dim 2112; the crate then switches to its i32 LUT mode); the bytes
    of both writers are refused by the library's RBQ1 reader, with no handle, and parsed as a valid stream by the host logic (the
    refusal is the build's limit, not a malformed stream)."""
    _, built = build_index(n=40, dim=2049, nlist=2, total_bits=bits, metric=metric, seed=2049 + bits)
    assert built.padded_dim == 2112
    for blob in (built.save_rbq1(), from_built(built)):
        rc, h, det = _load_rbq1(blob)
        assert (rc, h, det) == (CFG, None, TOO_WIDE)
        rc, det = _hostcheck(hostcheck.rbq_hostcheck_parse, blob)
        assert rc == 0, det  # (load_from_reader's own checks pass: validate_header refuses)
    # 2048 (the largest accepted padded_dim) still parses
    _, ok = build_index(n=40, dim=2047, nlist=2, total_bits=bits, metric=metric, seed=2047)
    assert _hostcheck(hostcheck.rbq_hostcheck_parse, ok.save_rbq1())[0] == 0


@pytest.mark.parametrize("metric,bits", [(0, 7), (1, 3)])
def test_rbf1_of_dim_2049_is_refused(metric, bits):
    rng = np.random.default_rng(2049)
    b = rq.builder.train_bruteforce(rng.standard_normal((12, 2049)).astype(np.float32), bits, metric, 1, 5, True)
    h, a = b.header, b.arrays()
    assert h.padded_dim == 2112
    blob = write_rbf1(h.dim, h.padded_dim, h.metric, h.rotator, h.ex_bits, b.rotator_blob(), a["bin"], a["ex"], a)
    assert _load_rbf1(blob) == (CFG, None, TOO_WIDE)


def _matrix_rbf1(dim, ex_bits=6, n=3):
    """an RBF1 stream of a Matrix-rotated index of any dim, written by hand (the CPU builder refuses such dims)"""
    R = np.linalg.qr(np.random.default_rng(dim).standard_normal((dim, dim)))[0].astype(np.float32)
    bin_codes = np.zeros((n, (dim + 7) // 8), np.uint8)
    ex_codes = np.zeros((n, (dim * ex_bits + 7) // 8), np.uint8)
    return write_rbf1(dim, dim, 0, 0, ex_bits, R.tobytes(), bin_codes, ex_codes, {f: np.ones(n, np.float32) for f in FACTORS})


@pytest.mark.parametrize("dim", [1, 7, 20, 24, 100, 2049])
def test_matrix_dim_not_multiple_of_16_is_refused(dim):
    """The Matrix rotator keeps padded_dim == dim; FastScan needs a multiple of 16 (the crate asserts it) and so do the packed
    ex-code layouts this build serves.  The crate has no message of its own for this (it asserts), so the CPU builders refuse such a
    dim with InvalidConfig and the device library's message (they used to write past the packed codes' buffers), and the RBQ1 / RBF1 readers refuse a hand-written stream of it with the reader's message, no handle."""
    data = np.random.default_rng(dim).standard_normal((40, dim)).astype(np.float32)
    for bits in (1, 3, 7):
        with pytest.raises(rq.RabitqError) as e:
            rq.builder.train_with_clusters(data, data[:2], np.zeros(40, np.uint32), bits, 0, 0, 1, True)
        assert (e.value.kind, e.value.detail) == ("InvalidConfig", NOT_16)
        with pytest.raises(rq.RabitqError) as e:
            rq.builder.train_bruteforce(data, bits, 0, 0, 1, True)
        assert (e.value.kind, e.value.detail) == ("InvalidConfig", NOT_16)
    R = np.linalg.qr(np.random.default_rng(dim).standard_normal((dim, dim)))[0].astype(np.float32)
    cl = {"centroid": [0.0] * dim, "ids": [0], "batch_data": bytes(dim * 4 + 384), "ex_codes": [bytes(dim * 6 // 8)],
          "f_add_ex": [0.0], "f_rescale_ex": [1.0], "delta": [1.0], "vl": [0.0]}
    assert _load_rbq1(write_rbq1(dim, dim, 0, 0, 6, R.tobytes(), [cl])) == (CFG, None, NOT_16)
    assert _load_rbf1(_matrix_rbf1(dim)) == (CFG, None, NOT_16)


def test_matrix_dims_of_the_table_still_build():
    """16, 80, 1008 and 2048 (multiples of 16) are built by both CPU builders"""
    for dim in MATRIX_DIMS:
        data = np.random.default_rng(dim).standard_normal((20, dim)).astype(np.float32)
        built = rq.builder.train_with_clusters(data, data[:2], np.zeros(20, np.uint32), 7, 0, 0, 1, True)
        assert built.padded_dim == dim
        assert rq.builder.train_bruteforce(data, 3, 1, 0, 1, True).header.padded_dim == dim


@pytest.mark.parametrize("dim", [1, 33, 2047])
def test_accepted_edge_dims_still_parse(dim):
    """below the bound the C++ writer and the independent writer agree byte for byte at dims 1, 33 and 2047"""
    _, built = build_index(n=40, dim=dim, nlist=2, total_bits=7, seed=dim)
    blob = built.save_rbq1()
    assert blob == from_built(built)
