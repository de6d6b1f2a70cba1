// km_common.hpp — what the GEMM-shortlist-rescore paths share (k_kmeans.hip: k-means assignment; k_mstg.hip: MSTG closure
// assignment): canonical norms, the split-bf16 image of a chunk of rows, the finite-input check, and the device workspace.
// The kernels are static: each unit that includes this header launches its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "kernels.hpp"

namespace rbq {

constexpr uint32_t kShortlist = 256;            // shortlist capacity per row
constexpr uint32_t kFallbackMark = 0xffffffffu; // shortlist length of a row that is scored against every centroid

__device__ __forceinline__ float km_norm(const float* __restrict__ x, uint32_t dim) {
    float s = 0.0f;
    for (uint32_t j = 0; j < dim; ++j) { const float p = x[j] * x[j]; s = s + p; }
    return s;
}

// any non-finite value in x[0, count) sets *bad
static __global__ __launch_bounds__(256) void k_km_nonfinite(const float* __restrict__ x, uint64_t count, uint32_t* __restrict__ bad) {
    bool b = false;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < count; i += (uint64_t)gridDim.x * 256u) b |= !isfinite(x[i]);
    if (__any(b) && (threadIdx.x & 63u) == 0) atomicOr(bad, 1u);
}

static __global__ __launch_bounds__(256) void k_km_norms(const float* __restrict__ x, uint64_t rows, uint32_t dim, float* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < rows) out[i] = km_norm(x + i * dim, dim);
}

// rows [0, nr) of x ([.][dim]) as bf16 hi / lo [nr][Dp], zero beyond dim
static __global__ __launch_bounds__(256) void k_km_split(const float* __restrict__ x, uint32_t nr, uint32_t dim, uint32_t Dp,
                                                  uint16_t* __restrict__ hi, uint16_t* __restrict__ lo) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= (uint64_t)nr * Dp) return;
    const uint64_t r = e / Dp;
    const uint32_t j = (uint32_t)(e - r * Dp);
    uint16_t h = 0, l = 0;
    if (j < dim) bf16_split(x[r * dim + j], h, l);
    hi[e] = h;
    lo[e] = l;
}

// centroid norms (lane per cluster) and their maximum (bit pattern of a non-negative float; reset to 0 by the caller)
static __global__ __launch_bounds__(256) void k_km_cnorms(const float* __restrict__ cent, uint32_t k, uint32_t dim, float* __restrict__ nc,
                                                   uint32_t* __restrict__ ncmax_bits) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= k) return;
    const float v = km_norm(cent + (size_t)c * dim, dim);
    nc[c] = v;
    atomicMax(ncmax_bits, __float_as_uint(v));
}

struct KmTemp { // device workspace freed on scope exit
    std::vector<void*> ptrs;
    template <class T> hipError_t alloc(T** p, size_t elems) {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, elems ? elems * sizeof(T) : 16);
        if (e == hipSuccess) { ptrs.push_back(q); *p = (T*)q; }
        return e;
    }
    ~KmTemp() { for (void* p : ptrs) (void)hipFree(p); }
};

// a failed HIP call ends the driver: RBQ_DEVICE with the call in `detail` (a std::string in scope)
#define KM_TRY(expr)                                                                                                     \
    do {                                                                                                                 \
        hipError_t _e = (expr);                                                                                          \
        if (_e != hipSuccess) { detail = std::string(#expr) + ": " + hipGetErrorString(_e); return RBQ_DEVICE; }          \
    } while (0)

inline unsigned grid_of(uint64_t n, unsigned b) { return (unsigned)((n + b - 1) / b); }

} // namespace rbq
