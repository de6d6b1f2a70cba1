// km_common.hpp — what the GEMM-shortlist-rescore paths share (k_kmeans.hip: k-means assignment; k_mstg.hip: MSTG closure
// assignment): canonical norms, the split-bf16 image of a chunk of rows, the finite-input check, and the device workspace.
// The kernels are static: each unit that includes this header launches its own copy.
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

// ---- the k-means kernels that k_kmeans.hip and k_hcluster.hip both launch
// canonical distance: sequential unfused dot in coordinate order, (nx + nc) - 2 dot, clamped to 0
__device__ __forceinline__ float km_canon(const float* __restrict__ x, const float* __restrict__ c, uint32_t dim, float nx, float nc) {
    float s = 0.0f;
    for (uint32_t j = 0; j < dim; ++j) { const float p = x[j] * c[j]; s = s + p; }
    float d = (nx + nc) - 2.0f * s;
    if (d < 0.0f) d = 0.0f;
    return d;
}

// one wavefront per row of the chunk: Amin, eps, shortlist (ascending cluster order) or the fallback mark
static __global__ __launch_bounds__(256) void k_km_scan(const float* __restrict__ dots, uint32_t nr, uint32_t k, uint32_t Dp,
                                                 const float* __restrict__ nx, const float* __restrict__ nc,
                                                 const uint32_t* __restrict__ ncmax_bits, uint32_t* __restrict__ sl,
                                                 uint32_t* __restrict__ sl_n, unsigned long long* __restrict__ stats) {
    const uint32_t lane = threadIdx.x & 63u, row = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (row >= nr) return;
    const float* d = dots + (size_t)row * k;
    const float x2 = nx[row];
    float amin = INFINITY;
    for (uint32_t c = lane; c < k; c += 64u) {
        const float a = fmaxf(fmaf(-2.0f, d[c], x2 + nc[c]), 0.0f);
        amin = fminf(amin, a);
    }
    for (int o = 32; o >= 1; o >>= 1) amin = fminf(amin, __shfl_xor(amin, o));
    const float span = x2 + __uint_as_float(*ncmax_bits);
    const float eps = ((float)Dp * 4.76837158203125e-07f + 6.103515625e-05f) * span * 1.0009765625f + 7.888609052210118e-31f;
    const float thr = amin + 2.01f * eps;
    uint32_t cnt = 0;
    bool over = !(span < 1e37f) || !(thr < 1e37f);
    for (uint32_t c0 = 0; c0 < k && !over; c0 += 64u) {
        const uint32_t c = c0 + lane;
        bool in = false;
        if (c < k) in = fmaxf(fmaf(-2.0f, d[c], x2 + nc[c]), 0.0f) <= thr;
        const unsigned long long m = __ballot(in);
        const uint32_t pos = cnt + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (in && pos < kShortlist) sl[(size_t)row * kShortlist + pos] = c;
        cnt += (uint32_t)__popcll(m);
        if (cnt > kShortlist) over = true;
    }
    if (lane == 0) {
        sl_n[row] = over ? kFallbackMark : cnt;
        if (over) atomicAdd(&stats[0], 1ull);
        else atomicMax(&stats[1], (unsigned long long)cnt);
    }
}

// one wavefront per row: canonical distances of the shortlisted clusters (lanes over the entries), or of all k clusters for a
// row marked by k_km_scan (lanes over the clusters).  The result is the min of (distance bits, cluster) over the non-NaN
// distances below +inf, which is what the strict < scan in cluster order from +inf picks (none: cluster 0, +inf).
static __global__ __launch_bounds__(256) void k_km_exact(const float* __restrict__ x, uint32_t nr, uint32_t dim, const float* __restrict__ nx,
                                                  const float* __restrict__ cent, const float* __restrict__ nc, uint32_t k,
                                                  const uint32_t* __restrict__ sl, const uint32_t* __restrict__ sl_n,
                                                  uint32_t* __restrict__ best, float* __restrict__ bestd) {
    const uint32_t lane = threadIdx.x & 63u, row = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (row >= nr) return;
    const float* xr = x + (size_t)row * dim;
    const uint32_t n = sl_n[row];
    const bool all = n == kFallbackMark;
    const uint32_t cnt = all ? k : n;
    const unsigned long long none = ((unsigned long long)__float_as_uint(INFINITY) << 32) | 0xffffffffull;
    unsigned long long key = none;
    for (uint32_t i = lane; i < cnt; i += 64u) {
        const uint32_t c = all ? i : sl[(size_t)row * kShortlist + i];
        const float v = km_canon(xr, cent + (size_t)c * dim, dim, nx[row], nc[c]);
        if (v < INFINITY) { // (not NaN, below +inf)
            const unsigned long long kv = ((unsigned long long)__float_as_uint(v) << 32) | c;
            key = kv < key ? kv : key;
        }
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o);
        key = other < key ? other : key;
    }
    if (lane == 0) {
        best[row] = key == none ? 0u : (uint32_t)key;
        if (bestd) bestd[row] = key == none ? INFINITY : __uint_as_float((uint32_t)(key >> 32));
    }
}

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

// Workspace and launches of the GEMM-shortlist assignment for up to R rows per pass against k centroids.
struct KmGemmAssign {
    uint64_t R = 0, k = 0;
    uint32_t dim = 0, Dp = 0;
    int device = 0;
    float *nc = nullptr, *dots = nullptr;
    uint32_t *ncmax = nullptr, *sl = nullptr, *sl_n = nullptr;
    uint16_t *xh = nullptr, *xl = nullptr, *ch = nullptr, *cl = nullptr;
    unsigned long long* stats = nullptr; // [2]: rows that fell back to every centroid, the largest shortlist
    // rows per pass for a problem of `rows` rows: scores (4k), split image (4 Dp) and shortlist per row within kKmeansChunkBytes
    static uint64_t chunk_rows(uint64_t rows, uint64_t k, uint32_t Dp) {
        const uint64_t per_row = 4 * k + 4ull * Dp + 4ull * kShortlist + 4;
        uint64_t r = (kKmeansChunkBytes / per_row) / 128 * 128;
        const uint64_t cap = g_km_chunk_rows_cap.load(std::memory_order_relaxed); // (test hook; 0: none)
        if (cap && cap / 128 * 128 < r) r = cap / 128 * 128; // (below 128: the floor that follows)
        r = r > 128 ? r : 128;
        const uint64_t all = (rows + 127) / 128 * 128;
        return r < all ? r : all;
    }
    hipError_t alloc(KmTemp& t, uint64_t rows, uint64_t k_, uint32_t dim_, int dev, hipStream_t s) {
        k = k_; dim = dim_; Dp = (dim + 31u) / 32u * 32u; device = dev;
        R = chunk_rows(rows, k, Dp);
        hipError_t e;
        if ((e = t.alloc(&nc, k)) || (e = t.alloc(&ncmax, 1)) || (e = t.alloc(&ch, k * Dp)) || (e = t.alloc(&cl, k * Dp)) ||
            (e = t.alloc(&dots, R * k)) || (e = t.alloc(&xh, R * Dp)) || (e = t.alloc(&xl, R * Dp)) ||
            (e = t.alloc(&sl, R * kShortlist)) || (e = t.alloc(&sl_n, R)) || (e = t.alloc(&stats, 2)))
            return e;
        return hipMemsetAsync(stats, 0, 16, s);
    }
    // centroid norms and their split image: before every assignment against new centroids
    hipError_t prep(const float* cent, hipStream_t s) {
        hipError_t e = hipMemsetAsync(ncmax, 0, 4, s);
        if (e) return e;
        hipLaunchKernelGGL(k_km_cnorms, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, s, cent, (uint32_t)k, dim, nc, ncmax);
        if ((e = hipGetLastError())) return e;
        hipLaunchKernelGGL(k_km_split, dim3((unsigned)((k * Dp + 255) / 256)), dim3(256), 0, s, cent, (uint32_t)k, dim, Dp, ch, cl);
        return hipGetLastError();
    }
    // assignment of rows [0, m) of xs (norms xn): best cluster (+ its distance when bd != null)
    hipError_t run(const float* xs, const float* xn, uint64_t m, const float* cent, uint32_t* out, float* bd, hipStream_t s) {
        for (uint64_t r0 = 0; r0 < m; r0 += R) {
            const uint32_t nr = (uint32_t)(m - r0 < R ? m - r0 : R);
            const float* xc = xs + r0 * dim;
            g_km_assign_passes.fetch_add(1, std::memory_order_relaxed);
            hipLaunchKernelGGL(k_km_split, dim3((unsigned)(((uint64_t)nr * Dp + 255) / 256)), dim3(256), 0, s, xc, nr, dim, Dp, xh, xl);
            hipError_t e = hipGetLastError();
            if (e) return e;
            RankParams p{};
            p.metric = 1; // inner products only: the norms are added by k_km_scan
            p.rot_hi = xh; p.rot_lo = xl; p.cent_hi = ch; p.cent_lo = cl;
            p.nq = nr; p.nlist = (uint32_t)k; p.D = Dp; p.scores = dots;
            p.split = true; p.wide = true; p.big = true; p.ksplit = 0;
            if ((e = launch_rank_gemm(p, device, s))) return e;
            hipLaunchKernelGGL(k_km_scan, dim3((nr + 3) / 4), dim3(256), 0, s, dots, nr, (uint32_t)k, Dp, xn + r0, nc, ncmax, sl, sl_n, stats);
            if ((e = hipGetLastError())) return e;
            hipLaunchKernelGGL(k_km_exact, dim3((nr + 3) / 4), dim3(256), 0, s, xc, nr, dim, xn + r0, cent, nc, (uint32_t)k, sl, sl_n,
                               out + r0, bd ? bd + r0 : nullptr);
            if ((e = hipGetLastError())) return e;
        }
        return hipSuccess;
    }
};

} // namespace rbq
