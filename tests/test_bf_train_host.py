"""rbq_bf_train_device / BruteForceRabitqIndex.train_on_device, the parts that need no GPU: the symbol and its declaration,
every argument error of the C entry (all raised before the first HIP call, each with a detail string), and the crate's
messages of the Python method in the crate's order."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rabitq_rs_amd as rq
from rabitq_rs_amd import bruteforce as bfm
from rabitq_rs_amd import index as ix
from conftest import ROOT

INVALID = rq._abi.RBQ_INVALID_CONFIG
CONST, OPTIMAL = rq._abi.RESCALE_CONST, rq._abi.RESCALE_OPTIMAL


def test_symbol_is_exported_and_declared():
    assert hasattr(bfm.lib(), "rbq_bf_train_device")
    hdr = open(os.path.join(ROOT, "include", "rbq_bf.h")).read()
    assert re.search(r"int rbq_bf_train_device\(const rbq_header\* hdr, const float\* data, uint64_t n, int rescale, float t_const,\s*"
                     r"uint64_t max_chunk_rows, int device, rbq_bf_index\*\* out\);", hdr)
    assert "src/brute_force.rs:214-285" in hdr


def header(dim=64, padded=64, rotator=1, ex_bits=6, metric=0):
    blob_len = 4 * padded // 8 if rotator == 1 else padded * padded * 4
    blob = (C.c_uint8 * max(blob_len, 1))()
    h = rq._abi.Header(dim, padded, metric, rotator, ex_bits, 0, 0, 0, C.cast(blob, C.POINTER(C.c_uint8)), blob_len)
    h._keep = blob
    return h


def call(h, data, n, rescale=CONST, t_const=1.5, chunk=0, out=True):
    handle = C.c_void_p(0xdead)
    rc = bfm.lib().rbq_bf_train_device(C.byref(h) if h is not None else None, data.ctypes.data if data is not None else None, n,
                                       rescale, t_const, chunk, -1, C.byref(handle) if out else None)
    if out:
        assert handle.value is None  # *out is cleared before anything else
    return rc, ix._detail()


DATA = np.zeros((4, 64), np.float32)


@pytest.mark.parametrize("case,want", [
    ("null_hdr", "null header"), ("null_data", "null data"), ("null_out", "null output"),
    ("empty", "training data must be non-empty"), ("rescale", "unknown rescale mode"), ("t_zero", "constant rescale factor"),
    ("t_negative", "constant rescale factor"), ("t_nan", "constant rescale factor"), ("ex3", "Unsupported ex_bits"),
    ("dim_not_16", "Dimension must be multiple of 16 for SIMD")])
def test_argument_errors_need_no_device(case, want):
    h = header()
    args = dict(h=h, data=DATA, n=4)
    if case == "null_hdr":
        args["h"] = None
    elif case == "null_data":
        args["data"] = None
    elif case == "null_out":
        args["out"] = False
    elif case == "empty":
        args["n"] = 0
    elif case == "rescale":
        args["rescale"] = 7
    elif case.startswith("t_"):
        args["t_const"] = {"t_zero": 0.0, "t_negative": -1.0, "t_nan": float("nan")}[case]
    elif case == "ex3":
        args["h"] = header(ex_bits=3)
    elif case == "dim_not_16":
        args["h"] = header(dim=40, padded=40, rotator=0)
        args["data"] = np.zeros((4, 40), np.float32)
    rc, detail = call(**args)
    assert rc == INVALID, (case, rc, detail)
    assert want in detail, (case, detail)


def test_empty_data_comes_before_the_header_checks():
    """the crate's order: empty data is reported even when the configuration is unservable too"""
    rc, detail = call(header(ex_bits=3), DATA, 0, rescale=7)
    assert (rc, detail) == (INVALID, "training data must be non-empty")


def test_unknown_rescale_is_refused_at_one_bit_too():
    rc, detail = call(header(ex_bits=0), DATA, 4, rescale=-1)
    assert rc == INVALID and "unknown rescale mode" in detail


@pytest.mark.parametrize("data", [np.zeros((0, 64), np.float32), np.zeros(0, np.float32), []], ids=["no-rows", "flat", "list"])
def test_python_empty_data_is_the_first_error(data):
    with pytest.raises(rq.RabitqError) as e:
        rq.BruteForceRabitqIndex.train_on_device(data, 0, 0, 1, 1, True)  # (total_bits is wrong too: empty data wins)
    assert e.value.kind == "InvalidConfig" and "training data must be non-empty" in str(e.value)


@pytest.mark.parametrize("bits", [0, 17])
def test_python_total_bits_range(bits):
    with pytest.raises(rq.RabitqError) as e:
        rq.BruteForceRabitqIndex.train_on_device(np.zeros((3, 40), np.float32), bits, 0, 0, 1, True)  # (dim 40 is unservable too)
    assert e.value.kind == "InvalidConfig" and "total_bits must be between 1 and 16" in str(e.value)


def test_python_unserved_configurations():
    with pytest.raises(rq.RabitqError, match="only 1, 3 and 7 total bits"):
        rq.BruteForceRabitqIndex.train_on_device(np.zeros((3, 64), np.float32), 4, 0, 1, 1, True)
    with pytest.raises(rq.RabitqError, match="multiple of 16"):
        rq.BruteForceRabitqIndex.train_on_device(np.zeros((3, 40), np.float32), 7, 0, 0, 1, True)


def test_builder_exposes_the_constant_rescale_factor():
    """train_on_device takes t_const from a one-row CPU build: it depends on (padded dim, bits, seed) only"""
    rng = np.random.default_rng(0)
    a = rq.builder.train_bruteforce(rng.standard_normal((1, 100)).astype(np.float32), 7, 0, 1, 9, True)
    b = rq.builder.train_bruteforce(rng.standard_normal((50, 128)).astype(np.float32), 7, 1, 1, 9, True)
    ivf = rq.builder.train_with_clusters(rng.standard_normal((2, 128)).astype(np.float32), np.zeros((1, 128), np.float32),
                                         np.zeros(2, np.uint32), 7, 0, 1, 9, True)
    assert a.t_const > 0 and a.t_const == b.t_const == ivf.t_const
    assert rq.builder.train_bruteforce(np.ones((1, 64), np.float32), 7, 0, 1, 9, False).t_const == 0.0
    assert rq.builder.train_bruteforce(np.ones((1, 64), np.float32), 1, 0, 1, 9, True).t_const == 0.0
