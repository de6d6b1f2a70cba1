// codes.hpp — decoders of the device code layout back into the crate's per-vector values, shared by the RBQ1 writer
// (k_save.hip) and fetch_embedding (k_fetch.hip).
//
//   dev_code_byte  byte `col` of a vector's packed sign code as unpack_single_vector (src/simd.rs:915-960) returns it:
//                  dimension 8 col + b is bit 7 - b (MSB first)
//   dev_ex_code    the ex code of one dimension as unpack_ex_code (src/simd.rs:101-131) returns it
#pragma once
#include "kernels.hpp"

namespace rbq {

// byte `col` of vector v's packed sign code in a device block (k_relayout_blocks' layout)
__device__ __forceinline__ uint32_t dev_code_byte(const uint8_t* __restrict__ blk, uint32_t G16, uint32_t col, uint32_t v) {
    const uint32_t g = col >> 4;
    return g < G16 ? blk[(size_t)g * 512 + v * 16 + (col & 15u)] : blk[(size_t)G16 * 512 + v * 8 + (col & 7u)];
}

// ex code of dimension i of a slot (lane l = i % 16 owns dims 16t + l; unit t / cpu holds code t % cpu at bit (t % cpu) * ex_bits)
__device__ __forceinline__ uint32_t dev_ex_code(const uint8_t* __restrict__ exs, uint32_t cpu, uint32_t ex_bits, uint32_t i) {
    const uint32_t t = i >> 4, l = i & 15u, unit = t / cpu, k = t - unit * cpu;
    const uint4 u = reinterpret_cast<const uint4*>(exs)[unit * 16 + l];
    const uint32_t bit = k * ex_bits, idx = bit >> 5, sh = bit & 31u;
    const uint32_t w0 = idx == 0 ? u.x : idx == 1 ? u.y : idx == 2 ? u.z : u.w;
    const uint32_t w1 = idx == 0 ? u.y : idx == 1 ? u.z : idx == 2 ? u.w : 0u;
    uint32_t raw = w0 >> sh;
    if (sh + ex_bits > 32) raw |= w1 << (32 - sh);
    return raw & ((1u << ex_bits) - 1u);
}

// ex code of dimension i of one vector's ex_code_packed as the brute-force index holds it (the cpp-compat packings, rbq_build.cpp
// pack_ex2 / pack_ex6): per 16 dimensions, 2 bits: 4 bytes, byte b bits 2g = dimension 4g + b; 6 bits: 12 bytes, byte b < 8 holds
// the low nibbles of dimensions b and b + 8, bytes 8-11 the top two bits laid out like the 2-bit packing
__device__ __forceinline__ uint32_t flat_ex_code(const uint8_t* __restrict__ row, uint32_t ex_bits, uint32_t i) {
    const uint32_t t = i >> 4, j = i & 15u, g = j >> 2, b = j & 3u;
    if (ex_bits == 2) return ((uint32_t)row[t * 4u + b] >> (2u * g)) & 3u;
    const uint8_t* u = row + t * 12u;
    const uint32_t lo = ((uint32_t)u[j & 7u] >> (j < 8u ? 0u : 4u)) & 15u;
    const uint32_t top = ((uint32_t)u[8u + b] >> (2u * g)) & 3u;
    return lo | (top << 4);
}

} // namespace rbq
