"""Raw vectors for the rerank kept as f16 or bf16 (option "rerank_raw_dtype"), what holds without a GPU:
the widening the kernels perform is the one torch performs on the CPU, for every bit pattern of both formats; the constants are
declared and mirrored and no entry point is added; a null handle is refused before anything else."""
import os

import numpy as np

from c_header import c_defines, c_functions
from conftest import ROOT
from rabitq_rs_amd import _abi
from rerank_f16_ref import BF16, F16, round_to, widen

HEADER = os.path.join(ROOT, "include", "rbq.h")


def test_widen_is_torch_float_on_every_bit_pattern():
    import torch
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    for dtype, tt in ((F16, torch.float16), (BF16, torch.bfloat16)):
        want = torch.from_numpy(bits.view(np.int16).copy()).view(tt).float().numpy()
        got = widen(bits, dtype)
        assert got.dtype == np.float32 and got.shape == bits.shape
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), dtype
        assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), dtype
        assert nan.sum() == (2046 if dtype == F16 else 254)  # 2 signs x (2^10 - 1 | 2^7 - 1) payloads
    assert widen(np.array([0x7E00], np.uint16), F16).view(np.uint32)[0] == 0x7FC00000  # the quiet NaNs the GPU tests carry
    assert widen(np.array([0x7FC0], np.uint16), BF16).view(np.uint32)[0] == 0x7FC00000


def test_round_to_is_the_nearest_pattern_and_widen_undoes_it():
    import torch
    rng = np.random.default_rng(2801)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32) * np.float32(10.0) ** rng.integers(-9, 5, 4096).astype(np.float32),
                        np.array([0.0, -0.0, np.inf, -np.inf, 65504.0, 65520.0, 1e-8, 3.3895314e38, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8],
                                 np.float32)])
    for dtype, tt in ((F16, torch.float16), (BF16, torch.bfloat16)):
        want = torch.from_numpy(x).to(tt).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(round_to(x, dtype), want), dtype
        bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
        w = widen(bits, dtype)
        ok = ~np.isnan(w)
        assert np.array_equal(round_to(w, dtype)[ok], bits[ok]), dtype  # every stored value is its own rounding
    assert round_to(np.array([np.nan], np.float32), F16)[0] & 0x7FFF == 0x7E00
    assert round_to(np.array([np.nan], np.float32), BF16)[0] == 0x7FC0


def test_the_dtype_travels_without_a_new_entry_point():
    """tests/test_abi_prototypes.py pins the entry points; the element type is the option "rerank_raw_dtype" of
    rbq_debug_set_option, read back through rbq_debug_copy_index, and its values are constants of rbq.h mirrored in _abi"""
    with open(HEADER) as f:
        text = f.read()
    functions, defines = c_functions(text), c_defines(text)
    assert (defines["RBQ_RAW_F32"], defines["RBQ_RAW_F16"], defines["RBQ_RAW_BF16"]) == (0, 1, 2)
    assert (_abi.RAW_F32, _abi.RAW_F16, _abi.RAW_BF16) == (0, 1, 2)
    assert _abi.RAW_DTYPES == {"f32": 0, "f16": 1, "bf16": 2}
    assert '"rerank_raw_dtype"' in text
    for name in ("rbq_index_set_rerank_vectors", "rbq_debug_set_option", "rbq_debug_copy_index"):
        assert name in functions and name in _abi.LIBRBQ_BY_HEADER["rbq.h"]
    assert not [n for n in functions if n not in _abi.LIBRBQ_BY_HEADER["rbq.h"]]


def test_abi_version_stays_2_2():
    from rabitq_rs_amd import index
    assert index.lib().rbq_abi_version() == (2 << 16) | 2


def test_null_handle():
    from rabitq_rs_amd import index
    L = index.lib()
    rows = np.zeros((2, 8), np.float16)
    out = np.full(1, 7, np.int32)
    for dtype in (_abi.RAW_F32, _abi.RAW_F16, _abi.RAW_BF16, 3, -1):
        assert L.rbq_debug_set_option(None, b"rerank_raw_dtype", dtype) == _abi.RBQ_INVALID_CONFIG
    assert L.rbq_index_set_rerank_vectors(None, rows.ctypes.data, 2) == _abi.RBQ_INVALID_CONFIG
    assert L.rbq_debug_copy_index(None, b"rerank_raw_dtype", out.ctypes.data, 4) == _abi.RBQ_INVALID_CONFIG and out[0] == 7
