// k_gemm_shortlist.hip — the front of every "nearest centroids of a chunk of rows" path (k-means and hierarchical clustering, the
// MSTG closure assignment, the MSTG list selection): the finite-input check, canonical norms, the split-bf16 images of rows and
// centroids, the ranking GEMM's approximate inner products; each path then has a scan kernel of its own (shortlist_collect,
// km_common.hpp) and scores the shortlist exactly.  Also the k-means scan and exact kernels and their driver KmGemmAssign.  gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "rbq.h"
#include "launch.hpp"
#include "kernels.hpp"
#include "km_common.hpp"

namespace rbq {

std::atomic<uint64_t> g_km_chunk_rows_cap{0}, g_km_assign_passes{0}; // launch.hpp

// any non-finite value in x[0, count) sets *bad
__global__ __launch_bounds__(256) void k_km_nonfinite(const float* __restrict__ x, uint64_t count, uint32_t* __restrict__ bad) {
    bool b = false;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < count; i += (uint64_t)gridDim.x * 256u) b |= !isfinite(x[i]);
    if (__any(b) && (threadIdx.x & 63u) == 0) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(256) void k_km_norms(const float* __restrict__ x, uint64_t rows, uint32_t dim, float* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < rows) out[i] = km_norm(x + i * dim, dim);
}

// rows [0, nr) of x ([.][dim]) as bf16 hi / lo [nr][Dp], zero beyond dim
__global__ __launch_bounds__(256) void k_km_split(const float* __restrict__ x, uint32_t nr, uint32_t dim, uint32_t Dp,
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
__global__ __launch_bounds__(256) void k_km_cnorms(const float* __restrict__ cent, uint32_t k, uint32_t dim, float* __restrict__ nc,
                                                   uint32_t* __restrict__ ncmax_bits) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= k) return;
    const float v = km_norm(cent + (size_t)c * dim, dim);
    nc[c] = v;
    atomicMax(ncmax_bits, __float_as_uint(v));
}

// canonical distance: sequential unfused dot in coordinate order, (nx + nc) - 2 dot, clamped to 0
__device__ __forceinline__ float km_canon(const float* __restrict__ x, const float* __restrict__ c, uint32_t dim, float nx, float nc) {
    float s = 0.0f;
    for (uint32_t j = 0; j < dim; ++j) { const float p = x[j] * c[j]; s = s + p; }
    float d = (nx + nc) - 2.0f * s;
    if (d < 0.0f) d = 0.0f;
    return d;
}

// one wavefront per row of the chunk: Amin, eps, shortlist (ascending cluster order) or the fallback mark
__global__ __launch_bounds__(256) void k_km_scan(const float* __restrict__ dots, uint32_t nr, uint32_t k, uint32_t Dp,
                                                 const float* __restrict__ nx, const float* __restrict__ nc,
                                                 const uint32_t* __restrict__ ncmax_bits, uint32_t* __restrict__ sl,
                                                 uint32_t* __restrict__ sl_n, unsigned long long* __restrict__ stats) {
    const uint32_t lane = threadIdx.x & 63u, row = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (row >= nr) return;
    const float* d = dots + (size_t)row * k;
    const float x2 = nx[row];
    float amin = INFINITY;
    for (uint32_t c = lane; c < k; c += 64u) amin = fminf(amin, km_approx_dist(d, nc, x2, c));
    for (int o = 32; o >= 1; o >>= 1) amin = fminf(amin, __shfl_xor(amin, o));
    const float span = x2 + __uint_as_float(*ncmax_bits);
    const float eps = ((float)Dp * 4.76837158203125e-07f + 6.103515625e-05f) * span * 1.0009765625f + 7.888609052210118e-31f;
    bool over = !(span < 1e37f);
    const uint32_t cnt = shortlist_collect(d, nc, x2, k, amin + 2.01f * eps, kShortlist, sl + (size_t)row * kShortlist, lane, over);
    if (lane == 0) {
        sl_n[row] = over ? kFallbackMark : cnt;
        if (over) atomicAdd(&stats[0], 1ull);
        else atomicMax(&stats[1], (unsigned long long)cnt);
    }
}

// one wavefront per row: canonical distances of the shortlisted clusters (lanes over the entries), or of all k clusters for a
// row marked by k_km_scan (lanes over the clusters).  The result is the min of (distance bits, cluster) over the non-NaN
// distances below +inf, which is what the strict < scan in cluster order from +inf picks (none: cluster 0, +inf).
__global__ __launch_bounds__(256) void k_km_exact(const float* __restrict__ x, uint32_t nr, uint32_t dim, const float* __restrict__ nx,
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
    key = cl_wave_min(key);
    if (lane == 0) {
        best[row] = key == none ? 0u : (uint32_t)key;
        if (bestd) bestd[row] = key == none ? INFINITY : __uint_as_float((uint32_t)(key >> 32));
    }
}

hipError_t nonfinite_sync(const float* x, uint64_t count, uint32_t* d_flag, hipStream_t s, bool* bad) {
    uint32_t h = 0;
    hipError_t e = hipMemsetAsync(d_flag, 0, 4, s);
    if (e) return e;
    hipLaunchKernelGGL(k_km_nonfinite, dim3((unsigned)std::min<uint64_t>(4096, grid_of(count, 256))), dim3(256), 0, s, x, count, d_flag);
    if ((e = hipGetLastError()) || (e = hipMemcpy(&h, d_flag, 4, hipMemcpyDeviceToHost))) return e;
    *bad = h != 0;
    return hipSuccess;
}

hipError_t launch_row_norms(const float* x, uint64_t rows, uint32_t dim, float* out, hipStream_t s) {
    hipLaunchKernelGGL(k_km_norms, dim3(grid_of(rows, 256)), dim3(256), 0, s, x, rows, dim, out);
    return hipGetLastError();
}

hipError_t launch_centroid_norms(const float* cent, const CentView& v, hipStream_t s) {
    hipError_t e = hipMemsetAsync(v.ncmax_bits, 0, 4, s);
    if (e) return e;
    hipLaunchKernelGGL(k_km_cnorms, dim3(grid_of(v.k, 256)), dim3(256), 0, s, cent, v.k, v.dim, v.nc, v.ncmax_bits);
    return hipGetLastError();
}

static hipError_t launch_split(const float* x, uint32_t nr, uint32_t dim, uint32_t Dp, uint16_t* hi, uint16_t* lo, hipStream_t s) {
    hipLaunchKernelGGL(k_km_split, dim3(grid_of((uint64_t)nr * Dp, 256)), dim3(256), 0, s, x, nr, dim, Dp, hi, lo);
    return hipGetLastError();
}

hipError_t launch_split_centroids(const float* cent, const CentView& v, hipStream_t s) {
    hipError_t e = launch_centroid_norms(cent, v, s);
    return e ? e : launch_split(cent, v.k, v.dim, v.Dp, v.hi, v.lo, s);
}

hipError_t launch_approx_dots(const float* x, uint32_t nr, uint32_t dim, const CentView& v, uint16_t* xh, uint16_t* xl, float* dots,
                              int device, hipStream_t s) {
    hipError_t e = launch_split(x, nr, dim, v.Dp, xh, xl, s);
    if (e) return e;
    // (planar hi / lo planes; the interleaved hi|lo image of hl_layout.hpp would be a change of this function alone)
    RankParams p{};
    p.metric = 1; // inner products only: the norms are added by the caller's scan kernel
    p.rot_hi = xh; p.rot_lo = xl; p.cent_hi = v.hi; p.cent_lo = v.lo;
    p.nq = nr; p.nlist = v.k; p.D = v.Dp; p.scores = dots;
    p.split = true; p.wide = true; p.big = true; p.ksplit = 0;
    return launch_rank_gemm(p, device, s);
}

// rows per pass for a problem of `rows` rows: gemm_shortlist_row_bytes per row within kKmeansChunkBytes
static uint64_t km_chunk_rows(uint64_t rows, uint64_t k, uint32_t Dp) {
    uint64_t r = (kKmeansChunkBytes / gemm_shortlist_row_bytes(k, Dp, kShortlist)) / 128 * 128;
    const uint64_t cap = g_km_chunk_rows_cap.load(std::memory_order_relaxed); // (test hook; 0: none)
    if (cap && cap / 128 * 128 < r) r = cap / 128 * 128; // (below 128: the floor that follows)
    r = r > 128 ? r : 128;
    const uint64_t all = (rows + 127) / 128 * 128;
    return r < all ? r : all;
}

hipError_t KmGemmAssign::alloc(KmTemp& t, uint64_t rows, uint64_t k, uint32_t dim, int dev, hipStream_t s) {
    cv.k = (uint32_t)k; cv.dim = dim; cv.Dp = km_dp(dim); device = dev;
    R = km_chunk_rows(rows, k, cv.Dp);
    hipError_t e;
    if ((e = t.alloc(&cv.nc, k)) || (e = t.alloc(&cv.ncmax_bits, 1)) || (e = t.alloc(&cv.hi, k * cv.Dp)) || (e = t.alloc(&cv.lo, k * cv.Dp)) ||
        (e = t.alloc(&dots, R * k)) || (e = t.alloc(&xh, R * cv.Dp)) || (e = t.alloc(&xl, R * cv.Dp)) ||
        (e = t.alloc(&sl, R * kShortlist)) || (e = t.alloc(&sl_n, R)) || (e = t.alloc(&stats, 2)))
        return e;
    return hipMemsetAsync(stats, 0, 16, s);
}

hipError_t KmGemmAssign::run(const float* xs, const float* xn, uint64_t m, const float* cent, uint32_t* out, float* bd, hipStream_t s) {
    hipError_t e = launch_split_centroids(cent, cv, s);
    for (uint64_t r0 = 0; r0 < m && !e; r0 += R) {
        const uint32_t nr = (uint32_t)(m - r0 < R ? m - r0 : R);
        const float* xc = xs + r0 * cv.dim;
        g_km_assign_passes.fetch_add(1, std::memory_order_relaxed);
        if ((e = launch_approx_dots(xc, nr, cv.dim, cv, xh, xl, dots, device, s))) return e;
        hipLaunchKernelGGL(k_km_scan, dim3((nr + 3) / 4), dim3(256), 0, s, dots, nr, cv.k, cv.Dp, xn + r0, cv.nc, cv.ncmax_bits, sl, sl_n, stats);
        if ((e = hipGetLastError())) return e;
        hipLaunchKernelGGL(k_km_exact, dim3((nr + 3) / 4), dim3(256), 0, s, xc, nr, cv.dim, xn + r0, cent, cv.nc, cv.k, sl, sl_n, out + r0,
                           bd ? bd + r0 : nullptr);
        e = hipGetLastError();
    }
    return e;
}

// TEST ONLY: what the drivers' front leaves behind, copied out pass by pass (nothing here is computed by other code than theirs)
int gemm_shortlist_front_tap(const FrontTapArgs& a, int device, std::string& detail) {
    const uint64_t n = a.n, k = a.k;
    const uint32_t dim = a.dim, Dp = km_dp(dim);
    const uint64_t R = km_chunk_rows(n, k, Dp);
    hipStream_t s = 0;
    KmTemp t;
    float *cent = nullptr, *d_in = nullptr, *nx = nullptr, *dots = nullptr;
    uint32_t* flag = nullptr;
    uint16_t *xh = nullptr, *xl = nullptr;
    CentView cv{(uint32_t)k, dim, Dp, nullptr, nullptr, nullptr, nullptr};
    KM_TRY(t.alloc(&flag, 1));
    KM_TRY(t.alloc(&cent, k * dim));
    KM_TRY(t.alloc(&cv.nc, k));
    KM_TRY(t.alloc(&cv.ncmax_bits, 1));
    KM_TRY(t.alloc(&cv.hi, k * Dp));
    KM_TRY(t.alloc(&cv.lo, k * Dp));
    KM_TRY(t.alloc(&d_in, R * dim));
    KM_TRY(t.alloc(&nx, R));
    KM_TRY(t.alloc(&xh, R * Dp));
    KM_TRY(t.alloc(&xl, R * Dp));
    KM_TRY(t.alloc(&dots, R * k));
    KM_TRY(hipMemcpy(cent, a.centroids, k * dim * 4, hipMemcpyHostToDevice));
    bool bad = false;
    KM_TRY(nonfinite_sync(cent, k * dim, flag, s, &bad));
    if (bad) { detail = "GEMM-shortlist front input must be finite"; return RBQ_INVALID_CONFIG; }
    KM_TRY(launch_split_centroids(cent, cv, s));
    KM_TRY(hipMemcpy(a.nc, cv.nc, k * 4, hipMemcpyDeviceToHost));
    KM_TRY(hipMemcpy(a.ncmax, cv.ncmax_bits, 4, hipMemcpyDeviceToHost));
    if (a.cent_hi) {
        KM_TRY(hipMemcpy(a.cent_hi, cv.hi, k * Dp * 2, hipMemcpyDeviceToHost));
        KM_TRY(hipMemcpy(a.cent_lo, cv.lo, k * Dp * 2, hipMemcpyDeviceToHost));
    }
    for (uint64_t r0 = 0; r0 < n; r0 += R) {
        const uint32_t nr = (uint32_t)(n - r0 < R ? n - r0 : R);
        KM_TRY(hipMemcpy(d_in, a.rows + r0 * dim, (size_t)nr * dim * 4, hipMemcpyHostToDevice));
        KM_TRY(nonfinite_sync(d_in, (uint64_t)nr * dim, flag, s, &bad));
        if (bad) { detail = "GEMM-shortlist front input must be finite"; return RBQ_INVALID_CONFIG; }
        KM_TRY(launch_row_norms(d_in, nr, dim, nx, s));
        KM_TRY(launch_approx_dots(d_in, nr, dim, cv, xh, xl, dots, device, s));
        KM_TRY(hipMemcpy(a.nx + r0, nx, (size_t)nr * 4, hipMemcpyDeviceToHost));
        KM_TRY(hipMemcpy(a.dots + r0 * k, dots, (size_t)nr * k * 4, hipMemcpyDeviceToHost));
        if (a.row_hi) {
            KM_TRY(hipMemcpy(a.row_hi + r0 * Dp, xh, (size_t)nr * Dp * 2, hipMemcpyDeviceToHost));
            KM_TRY(hipMemcpy(a.row_lo + r0 * Dp, xl, (size_t)nr * Dp * 2, hipMemcpyDeviceToHost));
        }
    }
    return RBQ_OK;
}

} // namespace rbq
