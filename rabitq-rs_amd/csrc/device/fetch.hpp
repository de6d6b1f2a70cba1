// fetch.hpp — what the fetch_embedding kernels of the IVF index (k_fetch.hip) and of the brute-force index (k_bf_mutate.hip)
// share: the FHT-Kac inverse rotation of one vector in LDS (inverse_rotate_into, src/rotation.rs:403-480), a workgroup per
// vector.  Every float operation is the crate's, one at a time and in its order (-ffp-contract=off keeps mul and add apart).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rbq {

constexpr uint32_t kFetchThreads = 256;
constexpr uint32_t kFetchMaxD = 2048; // validate_header's padded_dim bound: 8 KB of LDS per vector

__device__ __forceinline__ void lds_scale(float* s, uint32_t a, uint32_t e, float f) {
    for (uint32_t i = a + threadIdx.x; i < e; i += blockDim.x) s[i] = s[i] * f;
    __syncthreads();
}

// flip_sign with round r's flip bits (bit i % 8 of byte i / 8, LSB first)
__device__ __forceinline__ void lds_flip(float* s, uint32_t D, const uint8_t* __restrict__ flip) {
    for (uint32_t i = threadIdx.x; i < D; i += blockDim.x)
        if ((flip[i >> 3] >> (i & 7u)) & 1u) s[i] = -s[i];
    __syncthreads();
}

// fht over s[0, n), n a power of two: stage h pairs (j, j + h); every butterfly is (x + y, x - y)
__device__ __forceinline__ void lds_fht(float* s, uint32_t n) {
    for (uint32_t h = 1; h < n; h <<= 1) {
        for (uint32_t k = threadIdx.x; k < n / 2; k += blockDim.x) {
            const uint32_t j = ((k & ~(h - 1)) << 1) | (k & (h - 1));
            const float x = s[j], y = s[j + h];
            s[j] = x + y;
            s[j + h] = x - y;
        }
        __syncthreads();
    }
}

// kacs_walk over s[0, D)
__device__ __forceinline__ void lds_kac(float* s, uint32_t D) {
    const uint32_t half = D / 2;
    for (uint32_t i = threadIdx.x; i < half; i += blockDim.x) {
        const float x = s[i], y = s[i + half];
        s[i] = x + y;
        s[i + half] = x - y;
    }
    __syncthreads();
}

// inverse_rotate_into of the FHT-Kac rotator over s[0, D) (every thread of the workgroup calls it, after a barrier that follows
// the writes of s; it ends with one).  flips: the rotator's 4 x D / 8 flip bytes; T = trunc_dim; rfac = 1 / fac and rlen = 1 / T,
// the crate's f32 divisions, done on the host.
__device__ __forceinline__ void lds_inverse_fht_kac(float* s, uint32_t D, uint32_t T, float rfac, float rlen, const uint8_t* __restrict__ flips) {
    const uint32_t fo = D / 8;
    if (T == D) { // rounds 4..1: *= 1/fac, fht, *= 1/D, flip
        for (int r = 3; r >= 0; --r) {
            lds_scale(s, 0, D, rfac);
            lds_fht(s, D);
            lds_scale(s, 0, D, rlen);
            lds_flip(s, D, flips + r * fo);
        }
    } else {      // *= 4, then rounds 4..1: *= 0.5, kacs_walk, on the segment *= 1/fac, fht, *= 1/trunc, flip
        const uint32_t start = D - T;
        lds_scale(s, 0, D, 4.0f);
        for (int r = 3; r >= 0; --r) {
            const uint32_t a = (r & 1) ? start : 0u; // rounds 4 and 2: [start..]; 3 and 1: [..trunc]
            lds_scale(s, 0, D, 0.5f);
            lds_kac(s, D);
            lds_scale(s, a, a + T, rfac);
            lds_fht(s + a, T);
            lds_scale(s, a, a + T, rlen);
            lds_flip(s, D, flips + r * fo);
        }
    }
}

} // namespace rbq
