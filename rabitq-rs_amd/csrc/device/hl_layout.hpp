// hl_layout.hpp — where the split-bf16 operands of the ranking GEMM live in memory.  Plain C++ (no HIP header): the kernels that
// write the images, the host mirror behind the debug copies and tests/test_rank_lines_host.py all use this one mapping.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RBQ_HL_HD __host__ __device__
#else
#define RBQ_HL_HD
#endif

namespace rbq {

// Split-bf16 operand image of the ranking GEMM (k_rank_bf16_db): ONE array of 2 * D bf16 per row, hi | lo interleaved per
// K slab of 32 elements — slab s of a row is the 64 elements (128 bytes) at 64 * s: the hi values of elements 32s .. 32s+31,
// then their lo values, so that a slab's two planes are one aligned 128-byte line.  Returns the offset (in elements, inside
// the row) of element i of plane `plane` (0: hi, 1: lo).  A last slab shorter than 32 (D % 32 != 0: images the GEMM never
// reads) keeps hi | lo at its own width, which makes the mapping a bijection onto [0, 2 * D) for every D.
constexpr uint32_t kHlSlab = 32;
RBQ_HL_HD inline uint32_t hl_offset(uint32_t i, uint32_t plane, uint32_t D) {
    const uint32_t s = i / kHlSlab, left = D - s * kHlSlab, w = left < kHlSlab ? left : kHlSlab;
    return 2u * kHlSlab * s + plane * w + (i - s * kHlSlab);
}

} // namespace rbq
