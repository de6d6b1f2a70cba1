// k_kmeans.hip — Faiss-style k-means on the device: run_kmeans_with_config (reference src/kmeans.rs) in the pinned arithmetic of
// the CPU restatement rbq_build_kmeans_faiss (csrc/host/rbq_build.cpp), which this unit reproduces bit for bit.  gfx950 only.
//
// Assignment of a chunk of rows (no N x k score matrix: R rows at a time, R x k approximate scores):
//   k_km_split      the chunk's rows as split-bf16 hi / lo images, zero-padded to Dp = dim rounded up to 32
//   k_rank_bf16_db  (rank_mfma.hpp, the ranking GEMM's inner-product form, launched through launch_rank_gemm) dA(x, c)
//   k_km_scan       per row: A = max(0, fmaf(-2, dA, nx + nc)), Amin, shortlist {c : A(c) <= Amin + 2 eps} in cluster order;
//                   a shortlist over kShortlist entries (or a score far from finite) marks the row for the fallback
//   k_km_exact      one wavefront per row: canonical distances of the shortlist, or of all k clusters for a marked row (the
//                   fallback: counted, never approximated); the strict < scan's choice as a min of (distance, cluster)
// eps bounds |A - canonical|: both share s = fl(nx + nc) of the canonical norms, so
//   |A - C| <= 2 |dA - dC| + u (|s - 2 dA| + |s - 2 dC|) and max(., 0) is 1-Lipschitz;  |dC - P| <= gamma_dim S,
//   |dA - P| <= (3.01 * 2^-16 + 6 Dp u) S  with S = sum |x_i c_i| <= (|x|^2 + |c|^2) / 2  (rank_mfma.hpp: the dropped split terms,
//   3 Dp exact products accumulated even by a truncating adder), the last term <= 4 u (|x|^2 + |c|^2):
//   eps = (8 Dp u + 4 * 2^-16)(nx + max nc) * (1 + 2^-10) + 2^-100 covers all of it, margin and underflow included.
// The canonical minimum c* satisfies A(c*) <= C(c*) + eps <= C(argmin A) + eps <= Amin + 2 eps: it is always shortlisted, and ties at
// the minimum are all shortlisted, so the lowest of them wins as in the full scan.
// Update (training rows, stable radix sort of (cluster, row) pairs): k_km_bounds -> member range per cluster; k_km_update one lane per
// (cluster, coordinate) sums its members in ascending row order (or copies a reseed row); k_km_candidates the 8 first rows of each
// decode_block_size chunk under (distance desc, row asc).  Reseeding and the RNG run on the host (one small copy per iteration).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "rbq.h"
#include "launch.hpp"
#include "kernels.hpp"
#include "km_common.hpp"
#include "../host/rbq_rng.h"

namespace rbq {

constexpr uint32_t kCands = 8;                 // RESEED_CANDIDATES (src/kmeans.rs)

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
__global__ __launch_bounds__(256) void k_km_bounds(const uint32_t* __restrict__ key, uint32_t rows, uint32_t* __restrict__ start,
                                                   uint32_t* __restrict__ end) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= rows) return;
    const uint32_t c = key[i];
    if (i == 0 || key[i - 1] != c) start[c] = i;
    if (i + 1 == rows || key[i + 1] != c) end[c] = i + 1;
}

// one wavefront per chunk of dbs rows: the 8 largest keys (distance bits << 32 | ~row), 0 where the chunk has fewer rows
__global__ __launch_bounds__(64) void k_km_candidates(const float* __restrict__ bestd, uint32_t rows, uint32_t dbs,
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
__global__ __launch_bounds__(64) void k_km_update(const float* __restrict__ x, uint32_t dim, const uint32_t* __restrict__ rows_sorted,
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

// spherical: c *= 1 / sqrt(|c|^2) when |c|^2 > 0 (correctly rounded sqrt and division)
__global__ __launch_bounds__(256) void k_km_normalize(float* __restrict__ cent, uint32_t k, uint32_t dim) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= k) return;
    float* p = cent + (size_t)c * dim;
    const float n = km_norm(p, dim);
    if (n > 0.0f) {
        const float inv = 1.0f / sqrtf(n);
        for (uint32_t j = 0; j < dim; ++j) p[j] = p[j] * inv;
    }
}

// per row: sequential f64 sum of ((float)(x - c))^2
__global__ __launch_bounds__(256) void k_km_objrow(const float* __restrict__ x, uint64_t n, uint32_t dim, const uint32_t* __restrict__ asg,
                                                   const float* __restrict__ cent, double* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float* xr = x + i * dim;
    const float* cr = cent + (size_t)asg[i] * dim;
    double s = 0.0;
    for (uint32_t j = 0; j < dim; ++j) {
        const double dl = (double)(xr[j] - cr[j]);
        s = s + dl * dl;
    }
    out[i] = s;
}

// one wavefront: the sequential f64 sum of v[0..n) in ascending order (64 values per coalesced load, added one by one)
__global__ __launch_bounds__(64) void k_km_sum64(const double* __restrict__ v, uint64_t n, double* __restrict__ out) {
    const uint32_t lane = threadIdx.x;
    double s = 0.0;
    for (uint64_t b = 0; b < n; b += 64u) {
        const double mine = b + lane < n ? v[b + lane] : 0.0;
        const uint32_t cnt = n - b < 64u ? (uint32_t)(n - b) : 64u;
        const uint64_t bits = (uint64_t)__double_as_longlong(mine);
        const uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32);
        for (uint32_t l = 0; l < cnt; ++l) {
            const uint64_t w = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)hi, (int)l) << 32) |
                               (uint32_t)__builtin_amdgcn_readlane((int)lo, (int)l);
            s = s + __longlong_as_double((long long)w);
        }
    }
    if (lane == 0) *out = s;
}

namespace {

void km_shuffle(std::vector<uint32_t>& v, rbq_host::Rng& rng) {
    for (size_t i = v.size(); i-- > 1;) std::swap(v[i], v[rng.next() % (i + 1)]);
}

} // namespace

// Bytes of the per-chunk assignment workspace per row: scores (4k), split image (4 Dp), shortlist.
static uint64_t km_chunk_rows(uint64_t rows, uint64_t k, uint32_t Dp) {
    const uint64_t per_row = 4 * k + 4ull * Dp + 4ull * kShortlist + 4;
    uint64_t r = (kKmeansChunkBytes / per_row) / 128 * 128;
    r = std::max<uint64_t>(r, 128);
    return std::min<uint64_t>(r, (rows + 127) / 128 * 128);
}

int kmeans_device(const KMeansArgs& a, std::string& detail) {
    const uint64_t n = a.n, k = a.k;
    const uint32_t dim = a.dim, Dp = (dim + 31u) / 32u * 32u;
    hipStream_t s = 0;
    KmTemp t;
    {   // finite input only: the shortlist's error bound needs it (the crate does not check)
        uint32_t* bad = nullptr;
        uint32_t h_bad = 0;
        KM_TRY(t.alloc(&bad, 1));
        KM_TRY(hipMemsetAsync(bad, 0, 4, s));
        hipLaunchKernelGGL(k_km_nonfinite, dim3((unsigned)std::min<uint64_t>(4096, grid_of(n * dim, 256))), dim3(256), 0, s, a.data,
                           n * dim, bad);
        KM_TRY(hipGetLastError());
        KM_TRY(hipMemcpy(&h_bad, bad, 4, hipMemcpyDeviceToHost));
        if (h_bad) { detail = "k-means input must be finite"; return RBQ_INVALID_CONFIG; }
    }
    // ---- sampling (select_training_indices) on the host, the sample gathered on the device
    rbq_host::Rng sampling_rng(a.seed);
    const uint64_t kp = a.mppc && k > UINT64_MAX / a.mppc ? UINT64_MAX : k * a.mppc;
    const uint64_t target = std::max(std::min(n, kp), k);
    const float* x = a.data;
    const uint32_t rows = (uint32_t)target;
    uint32_t *d_src = nullptr, *d_start = nullptr, *d_end = nullptr;
    KM_TRY(t.alloc(&d_src, std::max<uint64_t>(k, target != n ? target : 0)));
    KM_TRY(t.alloc(&d_start, k));
    KM_TRY(t.alloc(&d_end, k));
    if (target != n) {
        std::vector<uint32_t> idx(n);
        for (uint64_t i = 0; i < n; ++i) idx[i] = (uint32_t)i;
        km_shuffle(idx, sampling_rng);
        idx.resize(target);
        std::sort(idx.begin(), idx.end());
        float* sample = nullptr;
        KM_TRY(t.alloc(&sample, (size_t)target * dim));
        KM_TRY(hipMemcpy(d_src, idx.data(), target * 4, hipMemcpyHostToDevice));
        // gather = k_km_update with every member range empty: row i of the sample copies data row idx[i]
        KM_TRY(hipMemsetAsync(d_start, 0, k * 4, s));
        KM_TRY(hipMemsetAsync(d_end, 0, k * 4, s));
        for (uint64_t r0 = 0; r0 < target; r0 += k) { // (src is indexed by "cluster": k rows per launch)
            const uint64_t nr = std::min<uint64_t>(k, target - r0);
            hipLaunchKernelGGL(k_km_update, dim3((unsigned)nr, grid_of(dim, 64)), dim3(64), 0, s, a.data, dim, (const uint32_t*)nullptr,
                               d_start, d_end, d_src + r0, sample + r0 * dim);
            KM_TRY(hipGetLastError());
        }
        x = sample;
    }
    // ---- workspace
    const uint64_t R = km_chunk_rows(std::max<uint64_t>(n, rows), k, Dp);
    const uint32_t dbs = (uint32_t)std::min<uint64_t>(a.dbs, rows); // (a chunk of at least all rows is one chunk)
    const uint64_t nchunks_c = (rows + dbs - 1) / dbs;
    unsigned kbits = 1;
    while (kbits < 32 && (1ull << kbits) < k) ++kbits; // sort keys < k
    float *nx = nullptr, *full_nx = nullptr, *bestd = nullptr, *cent = nullptr, *nc = nullptr, *dots = nullptr;
    uint32_t *asg = nullptr, *keys = nullptr, *vals_in = nullptr, *vals = nullptr, *sl = nullptr, *sl_n = nullptr, *ncmax = nullptr,
             *fin = nullptr;
    uint16_t *xh = nullptr, *xl = nullptr, *ch = nullptr, *cl = nullptr;
    unsigned long long *cands = nullptr, *stats = nullptr;
    double *objrow = nullptr, *obj = nullptr;
    KM_TRY(t.alloc(&nx, rows));
    KM_TRY(t.alloc(&full_nx, n));
    KM_TRY(t.alloc(&bestd, rows));
    KM_TRY(t.alloc(&asg, rows));
    KM_TRY(t.alloc(&keys, rows));
    KM_TRY(t.alloc(&vals_in, rows));
    KM_TRY(t.alloc(&vals, rows));
    KM_TRY(t.alloc(&fin, n));
    KM_TRY(t.alloc(&objrow, n));
    KM_TRY(t.alloc(&obj, 1));
    KM_TRY(t.alloc(&cent, k * dim));
    KM_TRY(t.alloc(&nc, k));
    KM_TRY(t.alloc(&ncmax, 1));
    KM_TRY(t.alloc(&ch, k * Dp));
    KM_TRY(t.alloc(&cl, k * Dp));
    KM_TRY(t.alloc(&dots, R * k));
    KM_TRY(t.alloc(&xh, R * Dp));
    KM_TRY(t.alloc(&xl, R * Dp));
    KM_TRY(t.alloc(&sl, R * kShortlist));
    KM_TRY(t.alloc(&sl_n, R));
    KM_TRY(t.alloc(&cands, nchunks_c * kCands));
    KM_TRY(t.alloc(&stats, 2));
    KM_TRY(hipMemsetAsync(stats, 0, 16, s));
    size_t sort_bytes = 0;
    KM_TRY(sort_pairs_u32(nullptr, &sort_bytes, asg, keys, vals_in, vals, rows, kbits, s));
    void* sort_tmp = nullptr;
    KM_TRY(t.alloc((unsigned char**)&sort_tmp, sort_bytes));
    KM_TRY(launch_iota(vals_in, rows, s));
    hipLaunchKernelGGL(k_km_norms, dim3(grid_of(rows, 256)), dim3(256), 0, s, x, (uint64_t)rows, dim, nx);
    KM_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_km_norms, dim3(grid_of(n, 256)), dim3(256), 0, s, a.data, n, dim, full_nx);
    KM_TRY(hipGetLastError());

    auto prep_centroids = [&]() -> int {
        KM_TRY(hipMemsetAsync(ncmax, 0, 4, s));
        hipLaunchKernelGGL(k_km_cnorms, dim3(grid_of(k, 256)), dim3(256), 0, s, cent, (uint32_t)k, dim, nc, ncmax);
        KM_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_km_split, dim3(grid_of(k * Dp, 256)), dim3(256), 0, s, cent, (uint32_t)k, dim, Dp, ch, cl);
        KM_TRY(hipGetLastError());
        return RBQ_OK;
    };
    // assignment of rows [0, m) of xs (norms xn): best cluster (+ its distance when bd != null)
    auto assign = [&](const float* xs, const float* xn, uint64_t m, uint32_t* out, float* bd) -> int {
        for (uint64_t r0 = 0; r0 < m; r0 += R) {
            const uint32_t nr = (uint32_t)std::min<uint64_t>(R, m - r0);
            const float* xc = xs + r0 * dim;
            hipLaunchKernelGGL(k_km_split, dim3(grid_of((uint64_t)nr * Dp, 256)), dim3(256), 0, s, xc, nr, dim, Dp, xh, xl);
            KM_TRY(hipGetLastError());
            RankParams p{};
            p.metric = 1; // inner products only: the norms are added by k_km_scan
            p.rot_hi = xh; p.rot_lo = xl; p.cent_hi = ch; p.cent_lo = cl;
            p.nq = nr; p.nlist = (uint32_t)k; p.D = Dp; p.scores = dots;
            p.split = true; p.wide = true; p.big = true; p.ksplit = 0;
            KM_TRY(launch_rank_gemm(p, a.device, s));
            hipLaunchKernelGGL(k_km_scan, dim3(grid_of(nr, 4)), dim3(256), 0, s, dots, nr, (uint32_t)k, Dp, xn + r0, nc, ncmax, sl, sl_n,
                               stats);
            KM_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_km_exact, dim3(grid_of(nr, 4)), dim3(256), 0, s, xc, nr, dim, xn + r0, cent, nc, (uint32_t)k, sl, sl_n,
                               out + r0, bd ? bd + r0 : nullptr);
            KM_TRY(hipGetLastError());
        }
        return RBQ_OK;
    };

    std::vector<uint32_t> h_start(k), h_end(k), h_src(k);
    std::vector<unsigned long long> h_cands(nchunks_c * kCands), pool;
    double best_obj = 0.0;
    uint64_t st_reseed = 0, st_draws = 0;
    int rc;
    for (uint64_t r = 0; r < a.nredo; ++r) {
        rbq_host::Rng redo_rng(a.seed + r * 0x9e3779b97f4a7c15ull);
        {   // Forgy: centroid c = training row idx[c] (k_km_update with every member range empty)
            std::vector<uint32_t> idx(rows);
            for (uint32_t i = 0; i < rows; ++i) idx[i] = i;
            km_shuffle(idx, redo_rng);
            KM_TRY(hipMemcpy(d_src, idx.data(), k * 4, hipMemcpyHostToDevice));
            KM_TRY(hipMemsetAsync(d_start, 0, k * 4, s));
            KM_TRY(hipMemsetAsync(d_end, 0, k * 4, s));
            hipLaunchKernelGGL(k_km_update, dim3((unsigned)k, grid_of(dim, 64)), dim3(64), 0, s, x, dim, (const uint32_t*)nullptr, d_start,
                               d_end, d_src, cent);
            KM_TRY(hipGetLastError());
        }
        for (uint64_t it = 0; it < a.niter; ++it) {
            if ((rc = prep_centroids())) return rc;
            if ((rc = assign(x, nx, rows, asg, bestd))) return rc;
            KM_TRY(sort_pairs_u32(sort_tmp, &sort_bytes, asg, keys, vals_in, vals, rows, kbits, s));
            KM_TRY(hipMemsetAsync(d_start, 0, k * 4, s));
            KM_TRY(hipMemsetAsync(d_end, 0, k * 4, s));
            hipLaunchKernelGGL(k_km_bounds, dim3(grid_of(rows, 256)), dim3(256), 0, s, keys, rows, d_start, d_end);
            KM_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_km_candidates, dim3((unsigned)nchunks_c), dim3(64), 0, s, bestd, rows, dbs, cands);
            KM_TRY(hipGetLastError());
            KM_TRY(hipMemcpyAsync(h_start.data(), d_start, k * 4, hipMemcpyDeviceToHost, s));
            KM_TRY(hipMemcpyAsync(h_end.data(), d_end, k * 4, hipMemcpyDeviceToHost, s));
            KM_TRY(hipMemcpyAsync(h_cands.data(), cands, nchunks_c * kCands * 8, hipMemcpyDeviceToHost, s));
            KM_TRY(hipStreamSynchronize(s));
            // update_centroids' reseeding: empty clusters in ascending order take the pool's next candidate, then the RNG
            pool.clear();
            for (unsigned long long v : h_cands)
                if (v) pool.push_back(v);
            std::sort(pool.begin(), pool.end(), std::greater<unsigned long long>());
            size_t next = 0;
            bool any = false;
            for (uint64_t c = 0; c < k; ++c) {
                h_src[c] = 0;
                if (h_end[c] > h_start[c]) continue;
                any = true;
                ++st_reseed;
                if (next < pool.size()) h_src[c] = 0xffffffffu - (uint32_t)(pool[next++] & 0xffffffffull);
                else { h_src[c] = (uint32_t)(redo_rng.next() % rows); ++st_draws; }
            }
            if (any) KM_TRY(hipMemcpy(d_src, h_src.data(), k * 4, hipMemcpyHostToDevice));
            hipLaunchKernelGGL(k_km_update, dim3((unsigned)k, grid_of(dim, 64)), dim3(64), 0, s, x, dim, vals, d_start, d_end, d_src, cent);
            KM_TRY(hipGetLastError());
            if (a.spherical) {
                hipLaunchKernelGGL(k_km_normalize, dim3(grid_of(k, 256)), dim3(256), 0, s, cent, (uint32_t)k, dim);
                KM_TRY(hipGetLastError());
            }
        }
        // assignment of the full dataset and the objective
        if ((rc = prep_centroids())) return rc;
        if ((rc = assign(a.data, full_nx, n, fin, nullptr))) return rc;
        hipLaunchKernelGGL(k_km_objrow, dim3(grid_of(n, 256)), dim3(256), 0, s, a.data, n, dim, fin, cent, objrow);
        KM_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_km_sum64, dim3(1), dim3(64), 0, s, objrow, n, obj);
        KM_TRY(hipGetLastError());
        double o = 0.0;
        KM_TRY(hipMemcpy(&o, obj, 8, hipMemcpyDeviceToHost));
        if (r == 0 || o < best_obj) {
            best_obj = o;
            KM_TRY(hipMemcpy(a.centroids, cent, k * dim * 4, hipMemcpyDeviceToHost));
            KM_TRY(hipMemcpy(a.assignments, fin, n * 4, hipMemcpyDeviceToDevice));
        }
    }
    unsigned long long st[2];
    KM_TRY(hipMemcpy(st, stats, 16, hipMemcpyDeviceToHost));
    *a.objective = best_obj;
    if (a.stats) { a.stats[0] = st[0]; a.stats[1] = st_reseed; a.stats[2] = st_draws; a.stats[3] = st[1]; }
    return RBQ_OK;
}

} // namespace rbq
