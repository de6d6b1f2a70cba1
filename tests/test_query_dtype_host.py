"""Queries in f16 / bf16 (option "query_dtype"), what holds without a GPU: the marshalling of a query argument
(every accepted input, its code, the object that keeps the pointer alive, the refusals), the header's statement of the option and
the contract, the refusal through a null handle, and the byte arithmetic on query rows (rbq_host::QueryRows) in a stand-alone
program under AddressSanitizer + UBSan — nothing sanitized is loaded into this process."""
import os
import subprocess

import numpy as np
import pytest

from c_header import c_defines, c_functions
from conftest import ROOT
from rabitq_rs_amd import RabitqError, _abi, _marshal
from rerank_f16_ref import BF16, F16, round_to, widen

HEADER = os.path.join(ROOT, "include", "rbq.h")


# ---- _marshal.query_arg --------------------------------------------------------------------------------------------------------
def test_numpy_inputs_and_codes():
    x = np.arange(12, dtype=np.float32).reshape(3, 4)
    q, code = _marshal.query_arg(x)
    assert code == _abi.RAW_F32 and q is x and _marshal.data_ptr(q) == x.ctypes.data  # (as today: used in place)
    q, code = _marshal.query_arg(x[:, ::2])  # not contiguous: copied
    assert code == _abi.RAW_F32 and q.flags.c_contiguous and q.dtype == np.float32 and np.array_equal(q, x[:, ::2])
    q, code = _marshal.query_arg([[1, 2], [3, 4]])  # a list, float64, ints: f32 as today
    assert code == _abi.RAW_F32 and q.dtype == np.float32 and q.shape == (2, 2)
    q, code = _marshal.query_arg(x.astype(np.float64))
    assert code == _abi.RAW_F32 and q.dtype == np.float32
    h = x.astype(np.float16)
    q, code = _marshal.query_arg(h)
    assert code == _abi.RAW_F16 and q is h and q.itemsize == 2
    for name, c in ((F16, _abi.RAW_F16), (BF16, _abi.RAW_BF16)):
        bits = round_to(x, name)
        q, code = _marshal.query_arg(bits, dtype=name)
        assert code == c and q is bits and q.dtype == np.uint16
        q, code = _marshal.query_arg(bits, dtype=c)  # the RBQ_RAW_* value itself
        assert code == c
        assert np.array_equal(widen(q, name), x)  # (small integers: exact in both formats)
    q, code = _marshal.query_arg(x, dtype="f16")  # the caller's rounding, as set_rerank_vectors does it
    assert code == _abi.RAW_F16 and q.dtype == np.float16 and np.array_equal(q.view(np.uint16), round_to(x, F16))
    q, code = _marshal.query_arg(h, dtype="f32")
    assert code == _abi.RAW_F32 and q.dtype == np.float32 and np.array_equal(q, x)
    one, code = _marshal.query_arg(h[0])
    assert one.ndim == 1 and code == _abi.RAW_F16


def test_numpy_refusals():
    bits = np.zeros((2, 4), np.uint16)
    for bad in (None, "f32", _abi.RAW_F32):
        with pytest.raises(RabitqError) as e:
            _marshal.query_arg(bits, dtype=bad)
        assert e.value.code == _abi.RBQ_INVALID_CONFIG and "uint16" in str(e.value)
    with pytest.raises(RabitqError) as e:
        _marshal.query_arg(np.zeros((2, 4), np.float32), dtype="bf16")
    assert e.value.code == _abi.RBQ_INVALID_CONFIG
    for bad in ("f64", "half", 3, -1):
        with pytest.raises(RabitqError) as e:
            _marshal.query_arg(np.zeros((2, 4), np.float32), dtype=bad)
        assert e.value.code == _abi.RBQ_INVALID_CONFIG


def test_torch_host_tensors():
    import torch
    x = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    q, code = _marshal.query_arg(x)
    assert code == _abi.RAW_F32 and q.data_ptr() == x.data_ptr() == _marshal.data_ptr(q) and not _marshal.on_device(q)
    for tt, c, name in ((torch.float16, _abi.RAW_F16, F16), (torch.bfloat16, _abi.RAW_BF16, BF16)):
        t = x.to(tt)
        q, code = _marshal.query_arg(t)
        assert code == c and q.data_ptr() == t.data_ptr() and q.dtype == tt and q.element_size() == 2
        q, code = _marshal.query_arg(t.t())  # not contiguous: copied, the type kept
        assert code == c and q.is_contiguous() and q.dtype == tt and q.shape == (4, 3)
        bits = q.view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(widen(bits, name), x.t().numpy())
        q, code = _marshal.query_arg(t, dtype="f32")
        assert code == _abi.RAW_F32 and q.dtype == torch.float32 and torch.equal(q, x)
    q, code = _marshal.query_arg(x.double())
    assert code == _abi.RAW_F32 and q.dtype == torch.float32
    q, code = _marshal.query_arg(x, dtype="bf16")  # the caller asks torch to round
    assert code == _abi.RAW_BF16 and q.dtype == torch.bfloat16


# ---- the header ----------------------------------------------------------------------------------------------------------------
def test_header_names_the_option_and_the_contract():
    with open(HEADER) as f:
        text = f.read()
    functions, defines = c_functions(text), c_defines(text)
    assert (defines["RBQ_RAW_F32"], defines["RBQ_RAW_F16"], defines["RBQ_RAW_BF16"]) == (0, 1, 2)
    assert sorted(k for k in defines if k.startswith("RBQ_RAW_")) == ["RBQ_RAW_BF16", "RBQ_RAW_F16", "RBQ_RAW_F32"]  # no new #define
    assert "element types of 16-bit rows" in text
    assert text.count('"query_dtype"') >= 3  # the option list, rbq_search_batch, the read-back
    flat = " ".join(text.replace("*", " ").split())
    assert ("ids, counts, score bits, diag, list outputs and errors of a call with 16-bit queries equal those of the same call with "
            '"query_dtype" RBQ_RAW_F32 on the rows widened to f32') in flat
    assert flat.count("equal those of the same call with") >= 2  # at rbq_search_batch and in the option list
    assert "queries: pointer not aligned to its 16-bit elements" in text
    assert "in flight" in text
    assert not [n for n in functions if n not in _abi.LIBRBQ_BY_HEADER["rbq.h"]]  # no entry point was added for it


def test_null_handle():
    from rabitq_rs_amd import index
    L = index.lib()
    out = np.full(1, 7, np.int32)
    for v in (_abi.RAW_F32, _abi.RAW_F16, _abi.RAW_BF16, 3, -1):
        assert L.rbq_debug_set_option(None, b"query_dtype", v) == _abi.RBQ_INVALID_CONFIG
    assert L.rbq_debug_copy_index(None, b"query_dtype", out.ctypes.data, 4) == _abi.RBQ_INVALID_CONFIG and out[0] == 7


# ---- rbq_host::QueryRows under the sanitizers ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def querycheck(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("querycheck") / "querycheck")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "rabitq-rs_amd", "csrc", "host"), os.path.join(ROOT, "tests", "querycheck_main.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    return exe


def plan_ref(nq, forced):
    """subbatch_plan restated (rbq_host_logic.hpp)"""
    if forced:
        return [(q0, min(forced, nq - q0)) for q0 in range(0, nq, forced)]
    if nq < 256:
        return [(0, nq)] if nq else []
    if nq <= 2048:
        out, left, pos = [], nq, 0
        for i, w in enumerate((4, 3, 2, 1)):
            take = left if i == 3 else min(left, (nq * w // 10 + 31) // 32 * 32)
            if take:
                out.append((pos, take))
            pos, left = pos + take, left - take
        return out
    return [(q0, min(1024, nq - q0)) for q0 in range(0, nq, 1024)]


CASES = [(dt, dim, nq, forced, R) for dt in (0, 1, 2) for dim, nq, forced, R in
         ((960, 1024, 0, 1), (7, 300, 64, 2), (101, 10, 0, 3), (64, 7, 3, 4), (1, 5000, 0, 8), (2048, 1, 0, 1), (100, 2049, 0, 5))]


def test_row_offsets_of_sub_batches_and_shards(querycheck, tmp_path):
    path = tmp_path / "cases.txt"
    path.write_text("".join("%d %d %d %d %d\n" % c for c in CASES))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([querycheck, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and not out.stderr, out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(CASES)
    for (dt, dim, nq, forced, R), line in zip(CASES, lines):
        row = dim * (4 if dt == 0 else 2)
        shards = " ".join("%d:%d" % ((r * nq // R) * row, ((r + 1) * nq // R - r * nq // R) * row) for r in range(R))
        subs = " ".join("%d:%d" % (q0 * row, n * row) for q0, n in plan_ref(nq, forced))
        want = "row %d | shards %s | subs %s | aligned 1 %d |" % (row, shards, subs, 1 if dt == 0 else 0)
        assert line.startswith(want), (line, want)
    # spelt out by hand: 10 rows of 101 elements over three replicas are shards of 3, 3 and 4 rows — 606, 606, 808 bytes of f16 at
    # 0, 606, 1212; as f32 twice that
    assert lines[CASES.index((1, 101, 10, 0, 3))].startswith("row 202 | shards 0:606 606:606 1212:808 | subs 0:2020 |")
    assert lines[CASES.index((0, 101, 10, 0, 3))].startswith("row 404 | shards 0:1212 1212:1212 2424:1616 | subs 0:4040 |")
    # forced sub-batches of 64 at 300 rows of 7 bf16 elements: 14 bytes a row, the last sub-batch 44 rows
    assert lines[CASES.index((2, 7, 300, 64, 2))].startswith("row 14 | shards 0:2100 2100:2100 | subs 0:896 896:896 1792:896 2688:896 3584:616 |")
