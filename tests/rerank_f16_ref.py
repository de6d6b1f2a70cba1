"""NumPy statement of the two 16-bit element types the rerank's raw rows may be kept in (RBQ_RAW_F16, RBQ_RAW_BF16; DESIGN.md
section 28): how the stored bits widen to f32 — exactly, which is all the library does — and how a caller rounds f32 data to
them (round to nearest even; the library never rounds)."""
import numpy as np

F16, BF16 = "f16", "bf16"


def widen(bits_u16, dtype):
    """the f32 value of every stored 16-bit pattern: binary16 converted (subnormals, zeros, infinities, NaNs), bf16 = bits << 16"""
    b = np.ascontiguousarray(bits_u16, np.uint16)
    if dtype == F16:
        return b.view(np.float16).astype(np.float32)
    if dtype == BF16:
        return (b.astype(np.uint32) << np.uint32(16)).view(np.float32)
    raise ValueError(dtype)


def round_to(x_f32, dtype):
    """the 16-bit pattern nearest to every f32 value, ties to even (NaN: a quiet NaN of the format)"""
    x = np.ascontiguousarray(x_f32, np.float32)
    if dtype == F16:
        with np.errstate(over="ignore"):  # (beyond 65520 the nearest value is the infinity)
            return x.astype(np.float16).view(np.uint16)
    if dtype == BF16:
        u = x.view(np.uint32)
        r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
        return np.where(np.isnan(x), np.uint16(0x7FC0), r)
    raise ValueError(dtype)
