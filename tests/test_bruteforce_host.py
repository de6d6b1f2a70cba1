"""Brute-force index (BruteForceRabitqIndex, reference src/brute_force.rs), the parts that need no GPU: the RBF1 reader and
writer of the host logic (csrc/host/rbq_host_logic.hpp through rbq_hostcheck.cpp) against an independent Python writer, every
error string of the reader, the CPU trainer's validation, the numpy restatement's self-checks, the sanitizer build, and the
instruction mix of the compiled kernels."""
import ctypes as C
import glob
import os
import re
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import rabitq_rs_amd as rq
from conftest import ROOT
from rbf1_writer import FACTORS, write_rbf1
import bf_ref

HOST = os.path.join(ROOT, "rabitq-rs_amd", "csrc", "host")


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostcheck") / "librbq_hostcheck.so")
    subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-O1", "-I", os.path.join(ROOT, "include"), "-shared", "-o", out,
                           os.path.join(HOST, "rbq_hostcheck.cpp")])
    L = C.CDLL(out)
    L.rbq_hostcheck_parse_rbf1.restype = C.c_int
    L.rbq_hostcheck_parse_rbf1.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def parse(L, blob):
    buf = (C.c_uint8 * max(len(blob), 1)).from_buffer_copy(bytes(blob) or b"\0")
    det = C.create_string_buffer(256)
    nv, cs, same = C.c_uint64(), C.c_uint64(), C.c_int(0)
    rc = L.rbq_hostcheck_parse_rbf1(buf, len(blob), det, 256, C.byref(nv), C.byref(cs), C.byref(same))
    return rc, det.value.decode(), nv.value, bool(same.value)


def trained(n=60, dim=64, bits=7, metric=0, rotator=1, seed=5):
    data = np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)
    return data, rq.builder.train_bruteforce(data, bits, metric, rotator, seed, True)


def independent_bytes(b):
    h, a = b.header, b.arrays()
    return write_rbf1(h.dim, h.padded_dim, h.metric, h.rotator, h.ex_bits, b.rotator_blob(), a["bin"], a["ex"], a)


@pytest.mark.parametrize("bits,metric,rotator,dim", [(7, 0, 1, 64), (3, 1, 1, 100), (7, 1, 0, 32), (3, 0, 0, 48), (7, 0, 1, 960)])
def test_rbf1_round_trip_and_independent_writer(hostcheck, bits, metric, rotator, dim):
    """the reader accepts the independent writer's stream, and the C++ writer (rbf1_write) re-creates it byte for byte from
    what the reader parsed: load(save(x)) == x"""
    _, b = trained(n=37, dim=dim, bits=bits, metric=metric, rotator=rotator)
    blob = independent_bytes(b)
    rc, det, nv, same = parse(hostcheck, blob)
    assert rc == 0, det
    assert nv == 37 and same


def test_one_bit_streams_are_refused_like_the_crate(hostcheck):
    """a freshly trained 1-bit index carries D/16*2 zero bytes of ex code per vector (quantizer.rs:212-219), the writer
    writes them and the reader reads none: "checksum mismatch" (the crate cannot load its own 1-bit files)"""
    _, b = trained(n=20, dim=64, bits=1)
    a = b.arrays()
    assert a["ex"].shape == (20, 64 // 8) and not a["ex"].any()
    rc, det, _, _ = parse(hostcheck, independent_bytes(b))
    assert (rc, det) == (rq._abi.RBQ_INVALID_PERSISTENCE, "checksum mismatch")
    # a 1-bit stream without those bytes (a loaded index, saved again) is read
    blob = write_rbf1(64, 64, 0, 1, 0, b.rotator_blob(), a["bin"], np.zeros((20, 0), np.uint8), a)
    rc, det, nv, same = parse(hostcheck, blob)
    assert rc == 0 and nv == 20 and same, det


def _restamp(body):
    return b"RBF1" + struct.pack("<I", 1) + body + struct.pack("<I", zlib.crc32(body) & 0xFFFFFFFF)


def test_every_reader_error(hostcheck):
    _, b = trained(n=5, dim=64, bits=7)
    good = independent_bytes(b)
    body = bytearray(good[8:-4])
    P, IO = rq._abi.RBQ_INVALID_PERSISTENCE, rq._abi.RBQ_IO

    def with_field(off, fmt, val):
        x = bytearray(body)
        struct.pack_into(fmt, x, off, val)
        return _restamp(bytes(x))
    cases = [
        (b"RBQ1" + good[4:], P, "unrecognized file header"),
        (good[:4] + struct.pack("<I", 2) + good[8:], P, "unsupported index format version"),
        (with_field(0, "<I", 0), P, "dimension must be positive"),
        (with_field(4, "<I", 32), P, "padded_dim must be >= dim"),
        (with_field(8, "<B", 2), P, "unknown metric tag"),
        (with_field(9, "<B", 7), P, "unknown rotator type tag"),
        (with_field(10, "<B", 17), P, "ex_bits out of range"),
        (with_field(11, "<B", 0), P, "total_bits out of range"),
        (with_field(11, "<B", 17), P, "total_bits out of range"),
        (with_field(11, "<B", 3), P, "total_bits does not match ex_bits"),
        (with_field(9, "<B", 0), P, "rotator matrix length mismatch"),
        (good[:-1], IO, "failed to fill whole buffer"),
        (good[:12], IO, "failed to fill whole buffer"),
        (good[:len(good) // 2], IO, "failed to fill whole buffer"),
        (with_field(12, "<Q", 1 << 60), IO, "failed to fill whole buffer"),
        (good[:-5] + bytes([good[-5] ^ 1]) + good[-4:], P, "checksum mismatch"),
        (good[:-1] + bytes([good[-1] ^ 0x80]), P, "checksum mismatch"),
    ]
    # FhtKac flip bits of the wrong length (the header says 64 dims: 32 bytes expected)
    x = bytearray(body[:20]) + struct.pack("<Q", 31) + bytes(body[28:28 + 31]) + bytes(body[28 + 32:])
    cases.append((_restamp(bytes(x)), P, "FHT rotator flip bits length mismatch"))
    for blob, code, msg in cases:
        rc, det, _, _ = parse(hostcheck, blob)
        assert (rc, det) == (code, msg), (msg, rc, det)
    assert parse(hostcheck, good)[0] == 0


def test_train_validation_in_the_crates_order():
    E = rq.RabitqError
    with pytest.raises(E, match="training data must be non-empty"):
        rq.builder.train_bruteforce(np.zeros((0, 8), np.float32), 0, 0, 1, 1, True)  # (empty data first, before total_bits)
    with pytest.raises(E, match="total_bits must be between 1 and 16"):
        rq.builder.train_bruteforce(np.zeros((3, 8), np.float32), 17, 0, 1, 1, True)
    with pytest.raises(E, match="total_bits must be between 1 and 16"):
        rq.builder.train_bruteforce(np.zeros((3, 8), np.float32), 0, 0, 1, 1, True)
    with pytest.raises(E) as e:
        rq.builder.train_bruteforce(np.zeros((3, 64), np.float32), 5, 0, 1, 1, True)
    assert e.value.code == rq._abi.RBQ_INVALID_CONFIG and "only 1, 3 and 7" in str(e.value)


def test_trainer_arrays_follow_the_quantiser():
    """zero centroid: residual_norm = |rotated vector|, codes are the sign bits of the rotated vector"""
    data, b = trained(n=9, dim=64, bits=7, rotator=1)
    a = b.arrays()
    for v in range(9):
        r = b.rotate(data[v])
        assert np.array_equal(bf_ref.unpack_bits(a["bin"][v:v + 1], 64)[0], (r >= 0).astype(np.uint8))
        assert np.isclose(a["residual_norm"][v], np.linalg.norm(r.astype(np.float64)), rtol=1e-5)


@pytest.mark.parametrize("ex", [2, 6])
def test_restatement_unpacks_the_builders_packing(ex):
    L = rq.builder.lib()
    rng = np.random.default_rng(ex)
    D = 96
    codes = rng.integers(0, 1 << ex, (4, D)).astype(np.uint16)
    packed = np.zeros((4, D * ex // 8), np.uint8)
    for v in range(4):
        c = np.ascontiguousarray(codes[v])
        getattr(L, "rbq_build_pack_ex_code_%dbit" % ex)(c.ctypes.data, packed[v].ctypes.data, D)
    assert np.array_equal(bf_ref.unpack_ex(packed, D, ex), codes)


@pytest.mark.parametrize("bits,metric", [(1, 0), (3, 1), (7, 0)])
def test_vectorised_restatement_matches_a_scalar_loop(bits, metric):
    data, b = trained(n=11, dim=64, bits=bits, metric=metric)
    prep = bf_ref.Prepared(b.hdr_ptr, b.arrays())
    for q in np.random.default_rng(3).standard_normal((3, 64)).astype(np.float32):
        assert np.array_equal(bf_ref.distances(prep, q).view(np.uint32), bf_ref.scalar_search(prep, q, 5).view(np.uint32))


def test_rbf1_parser_fuzzed_under_asan_ubsan():
    """the sanitized host logic parses mutated RBF1 streams (every byte of every record read back, then written again)"""
    from test_sanitizers import _san_env
    env = _san_env()
    _, b = trained(n=12, dim=64, bits=7)
    seeds = [independent_bytes(b), independent_bytes(trained(n=7, dim=32, bits=3, rotator=0)[1])]
    path = os.path.join(ROOT, "tests", "_san", "rbf1_seeds.bin")
    with open(path, "wb") as f:
        for s in seeds:
            f.write(struct.pack("<Q", len(s)) + s)
    code = (
        "import ctypes as C, os, random, struct, zlib\n"
        "L = C.CDLL(os.environ['RBQ_HOSTCHECK_LIB'])\n"
        "L.rbq_hostcheck_parse_rbf1.restype = C.c_int\n"
        "L.rbq_hostcheck_parse_rbf1.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]\n"
        f"raw = open({path!r}, 'rb').read()\n"
        "seeds, o = [], 0\n"
        "while o < len(raw):\n"
        "    n = struct.unpack_from('<Q', raw, o)[0]; seeds.append(raw[o + 8:o + 8 + n]); o += 8 + n\n"
        "rnd = random.Random(11)\n"
        "ok = 0\n"
        "for it in range(3000):\n"
        "    s = bytearray(rnd.choice(seeds))\n"
        "    k = rnd.randrange(4)\n"
        "    if k == 0: s = s[:rnd.randrange(len(s))]\n"
        "    elif k == 1:\n"
        "        for _ in range(rnd.randrange(1, 4)): s[rnd.randrange(len(s))] = rnd.randrange(256)\n"
        "    elif k == 2:\n"
        "        off = rnd.choice([8, 12, 16, 17, 18, 19, 20, 28]); s[off:off + 1] = bytes([rnd.randrange(256)])\n"
        "    else:\n"
        "        off = rnd.choice([20, 28]); struct.pack_into('<Q', s, off, rnd.choice([0, 1, 2, 31, 33, 1 << 40, (1 << 64) - 1]))\n"
        "    if rnd.random() < 0.5 and len(s) > 12: s[-4:] = struct.pack('<I', zlib.crc32(bytes(s[8:-4])) & 0xffffffff)\n"
        "    buf = (C.c_uint8 * max(len(s), 1)).from_buffer_copy(bytes(s) or b'\\0')\n"
        "    det = C.create_string_buffer(256); a = C.c_uint64(); b = C.c_uint64(); same = C.c_int()\n"
        "    rc = L.rbq_hostcheck_parse_rbf1(buf, len(s), det, 256, C.byref(a), C.byref(b), C.byref(same))\n"
        "    ok += rc == 0\n"
        "    assert rc != 0 or same.value == 1\n"
        "print('fuzz ok', ok)\n")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    assert "fuzz ok" in out.stdout and "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr


def test_bf_kernels_have_no_fma_dot_or_scratch(tmp_path):
    """k_bf.hip compiled with the product flags: the BF kernels hold no v_fma* / v_fmac* / v_pk_fma* / v_dot* (the crate's
    sums are unfused) and use no scratch; the packed multiply / add carry the sums"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "rabitq-rs_amd", "csrc", "device", "k_bf.hip")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-gpu-rdc",
                           "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "--save-temps", "-c", src, "-o",
                           str(tmp_path / "k_bf.o")], cwd=str(tmp_path), stderr=subprocess.DEVNULL)
    asm = open(glob.glob(str(tmp_path / "*gfx950*.s"))[0]).read()
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN3rbq\w*k_bf\w*):[^\n]*\n(.*?)^\.Lfunc_end", asm, flags=re.M | re.S)}
    assert len(bodies) == 4, sorted(bodies)
    for name, body in bodies.items():
        bad = re.findall(r"^\s+(v_fma\w*|v_fmac\w*|v_pk_fma\w*|v_dot\w*|scratch_\w+|buffer_store\w*)", body, flags=re.M)
        assert not bad, (name, sorted(set(bad)))
    assert "v_pk_mul_f32" in bodies[[n for n in bodies if "k_bf_distILi6" in n][0]]
    for m in re.finditer(r"\.name:\s+(_ZN3rbq\S*k_bf\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", asm):
        assert int(m.group(2)) == 0, m.group(1)


def test_library_exports_every_brute_force_entry_point():
    from rabitq_rs_amd import index as ix
    from c_header import c_functions
    names = sorted(n for n in c_functions(open(os.path.join(ROOT, "include", "rbq_bf.h")).read()) if n.startswith("rbq_bf_"))
    assert len(names) >= 10, names
    lib = ix.lib()
    for n in names:
        assert hasattr(lib, n), n
    assert '#include "rbq_bf.h"' in open(os.path.join(ROOT, "include", "rbq.h")).read()
