// km_common.hpp — what the kernel units of the GEMM-shortlist-rescore paths inline (k_gemm_shortlist.hip: the shared front behind
// launch.hpp's launchers, and the k-means assignment; k_kmeans.hip; k_hcluster.hip; k_mstg.hip; k_mstg_search.hip): the canonical norm,
// the shortlist scans' approximate distance, error bound and collection loop, the drivers' device workspace, and KmGemmAssign.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "kernels.hpp"
#include "launch.hpp"

namespace rbq {

constexpr uint32_t kShortlist = 256;            // shortlist capacity per row
constexpr uint32_t kFallbackMark = 0xffffffffu; // shortlist length of a row that is scored against every centroid
constexpr uint32_t kCands = 8;                  // RESEED_CANDIDATES (src/kmeans.rs)

__device__ __forceinline__ float km_norm(const float* __restrict__ x, uint32_t dim) {
    float s = 0.0f;
    for (uint32_t j = 0; j < dim; ++j) { const float p = x[j] * x[j]; s = s + p; }
    return s;
}

// A(c) of the scans: the approximate squared distance from the GEMM's inner product d[c] (fmaxf drops a NaN: never negative, never
// NaN).  No __restrict__ here or on shortlist_collect: with it the scans' minimum loops are no longer unrolled (profiles/gemm_shortlist).
__device__ __forceinline__ float km_approx_dist(const float* d, const float* nc, float x2, uint32_t c) {
    return fmaxf(fmaf(-2.0f, d[c], x2 + nc[c]), 0.0f);
}

// eps of DESIGN.md section 15: |A - C| <= eps for the canonical C of math.rs's diff-squared form, span = nx + max nc, Dp <= 16384
__device__ __forceinline__ float closure_eps(uint32_t Dp, float span) {
    return ((float)(10u * Dp + 64u) * 5.9604644775390625e-08f + 6.103515625e-05f) * span * 1.015625f + 7.888609052210118e-31f;
}

// The shortlist {c : A(c) <= thr} of one row in centroid order, by the row's wavefront: the first `cap` entries go to sl_row and
// the count is returned.  `over` (the row is scored against every centroid instead) is set for a threshold near overflow or
// not finite and once the count passes cap, which ends the scan; a row that comes in with `over` set is not scanned.
__device__ __forceinline__ uint32_t shortlist_collect(const float* d, const float* nc, float x2, uint32_t k, float thr, uint32_t cap,
                                                      uint32_t* sl_row, uint32_t lane, bool& over) {
    uint32_t cnt = 0;
    bool o = over || !(thr < 1e37f); // (a local: carried through the loop, the reference costs scalar instructions per step)
    for (uint32_t c0 = 0; c0 < k && !o; c0 += 64u) {
        const uint32_t c = c0 + lane;
        bool in = false;
        if (c < k) in = km_approx_dist(d, nc, x2, c) <= thr;
        const unsigned long long m = __ballot(in);
        const uint32_t pos = cnt + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (in && pos < cap) sl_row[pos] = c;
        cnt += (uint32_t)__popcll(m);
        if (cnt > cap) o = true;
    }
    over = o;
    return cnt;
}

struct KmTemp { // device workspace freed on scope exit
    std::vector<void*> ptrs;
    size_t bytes = 0; // allocated so far
    template <class T> hipError_t alloc(T** p, size_t elems) {
        void* q = nullptr;
        const size_t want = elems ? elems * sizeof(T) : 16;
        hipError_t e = hipMalloc(&q, want);
        if (e == hipSuccess) { ptrs.push_back(q); *p = (T*)q; bytes += want; }
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

// ---- the k-means update step, which k_kmeans.hip and k_hcluster.hip both launch
// sorted cluster ids -> [start, end) of each cluster's members (both zeroed by the caller)
static __global__ __launch_bounds__(256) void k_km_bounds(const uint32_t* __restrict__ key, uint32_t rows, uint32_t* __restrict__ start,
                                                   uint32_t* __restrict__ end) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= rows) return;
    const uint32_t c = key[i];
    if (i == 0 || key[i - 1] != c) start[c] = i;
    if (i + 1 == rows || key[i + 1] != c) end[c] = i + 1;
}

// one wavefront per chunk of dbs rows: the 8 largest keys (distance bits << 32 | ~row), 0 where the chunk has fewer rows
static __global__ __launch_bounds__(64) void k_km_candidates(const float* __restrict__ bestd, uint32_t rows, uint32_t dbs,
                                                      unsigned long long* __restrict__ out) {
    const uint32_t lane = threadIdx.x, s0 = blockIdx.x * dbs, e = min(rows, s0 + dbs);
    unsigned long long t[kCands];
#pragma unroll
    for (uint32_t i = 0; i < kCands; ++i) t[i] = 0;
    for (uint32_t r = s0 + lane; r < e; r += 64u) {
        unsigned long long v = ((unsigned long long)__float_as_uint(bestd[r]) << 32) | (0xffffffffu - r);
#pragma unroll
        for (uint32_t i = 0; i < kCands; ++i) { // insertion into the descending list
            const unsigned long long a = t[i];
            t[i] = v > a ? v : a;
            v = v > a ? a : v;
        }
    }
    for (uint32_t round = 0; round < kCands; ++round) {
        unsigned long long m = t[0];
        for (int o = 32; o >= 1; o >>= 1) {
            const unsigned long long other = __shfl_xor(m, o);
            m = other > m ? other : m;
        }
        if (lane == 0) out[(size_t)blockIdx.x * kCands + round] = m;
        if (m != 0 && t[0] == m) { // the owner (keys are distinct) pops its head
#pragma unroll
            for (uint32_t i = 0; i + 1 < kCands; ++i) t[i] = t[i + 1];
            t[kCands - 1] = 0;
        }
    }
}

// one lane per (cluster, coordinate): sum of the members in ascending row order times 1 / count, or the reseed row
static __global__ __launch_bounds__(64) void k_km_update(const float* __restrict__ x, uint32_t dim, const uint32_t* __restrict__ rows_sorted,
                                                  const uint32_t* __restrict__ start, const uint32_t* __restrict__ end,
                                                  const uint32_t* __restrict__ src, float* __restrict__ cent) {
    const uint32_t c = blockIdx.x, j = blockIdx.y * 64u + threadIdx.x;
    if (j >= dim) return;
    const uint32_t b = start[c], e = end[c];
    float v;
    if (e > b) {
        float s = 0.0f;
        uint32_t m = b;
        for (; m + 4 <= e; m += 4) {
            const float v0 = x[(size_t)rows_sorted[m] * dim + j], v1 = x[(size_t)rows_sorted[m + 1] * dim + j];
            const float v2 = x[(size_t)rows_sorted[m + 2] * dim + j], v3 = x[(size_t)rows_sorted[m + 3] * dim + j];
            s = s + v0; s = s + v1; s = s + v2; s = s + v3;
        }
        for (; m < e; ++m) s = s + x[(size_t)rows_sorted[m] * dim + j];
        const float inv = 1.0f / (float)(e - b);
        v = s * inv;
    } else {
        v = x[(size_t)src[c] * dim + j];
    }
    cent[(size_t)c * dim + j] = v;
}

// math::l2_distance_sqr (AVX2 order, src/math.rs:216-245) by a group of 8 lanes: lane g of the group owns accumulator g.  Every
// lane of the group returns the distance.  All 64 lanes must call it together (a and b may be equal: a group with nothing to do).
__device__ __forceinline__ float cl_canon8(const float* a, const float* b, uint32_t dim, uint32_t lane) {
    const uint32_t g = lane & 7u, base = lane & ~7u, main = dim & ~7u;
    float acc = 0.0f;
    for (uint32_t i = g; i < main; i += 8u) {
        const float d = a[i] - b[i];
        const float p = d * d;
        acc = acc + p;
    }
    float sum = 0.0f;
    if (main) {
        sum = -0.0f;
#pragma unroll
        for (uint32_t l = 0; l < 8u; ++l) sum = sum + __shfl(acc, (int)(base + l));
    }
    for (uint32_t i = main; i < dim; ++i) {
        const float d = a[i] - b[i];
        const float p = d * d;
        sum = sum + p;
    }
    return sum;
}

__device__ __forceinline__ unsigned long long cl_wave_min(unsigned long long v) {
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long other = __shfl_xor(v, o);
        v = other < v ? other : v;
    }
    return v;
}

// The k-means assignment (k_gemm_shortlist.hip): workspace and launches for up to R rows per pass against k centroids.
struct KmGemmAssign {
    uint64_t R = 0;
    int device = 0;
    CentView cv{};
    float* dots = nullptr;
    uint32_t *sl = nullptr, *sl_n = nullptr;
    uint16_t *xh = nullptr, *xl = nullptr;
    unsigned long long* stats = nullptr; // [2]: rows that fell back to every centroid, the largest shortlist
    hipError_t alloc(KmTemp& t, uint64_t rows, uint64_t k, uint32_t dim, int dev, hipStream_t s);
    // assignment of rows [0, m) of xs (norms xn) to `cent`, prepared first: best cluster (+ its distance when bd != null)
    hipError_t run(const float* xs, const float* xn, uint64_t m, const float* cent, uint32_t* out, float* bd, hipStream_t s);
};

} // namespace rbq
