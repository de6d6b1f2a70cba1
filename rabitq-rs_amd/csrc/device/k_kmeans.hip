// k_kmeans.hip — Faiss-style k-means on the device: run_kmeans_with_config (reference src/kmeans.rs) in the pinned arithmetic of
// the CPU restatement rbq_build_kmeans_faiss (csrc/host/rbq_build.cpp), which this unit reproduces bit for bit.  gfx950 only.
//
// Assignment of a chunk of rows (KmGemmAssign, k_gemm_shortlist.hip; no N x k score matrix: R rows at a time, R x k approximate scores):
//   launch_approx_dots  the chunk's rows as split-bf16 hi / lo images, zero-padded to Dp = dim rounded up to 32, then dA(x, c) by
//                   the ranking GEMM's inner-product form (k_rank_bf16_db, rank_mfma.hpp)
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

int kmeans_device(const KMeansArgs& a, std::string& detail) {
    const uint64_t n = a.n, k = a.k;
    const uint32_t dim = a.dim;
    hipStream_t s = 0;
    KmTemp t;
    uint32_t* flag = nullptr; // finite input only: the shortlist's error bound needs it (the crate does not check)
    bool bad = false;
    KM_TRY(t.alloc(&flag, 1));
    KM_TRY(nonfinite_sync(a.data, n * dim, flag, s, &bad));
    if (bad) { detail = "k-means input must be finite"; return RBQ_INVALID_CONFIG; }
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
    const uint32_t dbs = (uint32_t)std::min<uint64_t>(a.dbs, rows); // (a chunk of at least all rows is one chunk)
    const uint64_t nchunks_c = (rows + dbs - 1) / dbs;
    unsigned kbits = 1;
    while (kbits < 32 && (1ull << kbits) < k) ++kbits; // sort keys < k
    float *nx = nullptr, *full_nx = nullptr, *bestd = nullptr, *cent = nullptr;
    uint32_t *asg = nullptr, *keys = nullptr, *vals_in = nullptr, *vals = nullptr, *fin = nullptr;
    unsigned long long* cands = nullptr;
    KmGemmAssign ga; // the assignment's workspace (k_gemm_shortlist.hip)
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
    KM_TRY(ga.alloc(t, std::max<uint64_t>(n, rows), k, dim, a.device, s));
    KM_TRY(t.alloc(&cands, nchunks_c * kCands));
    size_t sort_bytes = 0;
    KM_TRY(sort_pairs_u32(nullptr, &sort_bytes, asg, keys, vals_in, vals, rows, kbits, s));
    void* sort_tmp = nullptr;
    KM_TRY(t.alloc((unsigned char**)&sort_tmp, sort_bytes));
    KM_TRY(launch_iota(vals_in, rows, s));
    KM_TRY(launch_row_norms(x, rows, dim, nx, s));
    KM_TRY(launch_row_norms(a.data, n, dim, full_nx, s));

    std::vector<uint32_t> h_start(k), h_end(k), h_src(k);
    std::vector<unsigned long long> h_cands(nchunks_c * kCands), pool;
    double best_obj = 0.0;
    uint64_t st_reseed = 0, st_draws = 0;
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
            KM_TRY(ga.run(x, nx, rows, cent, asg, bestd, s));
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
        KM_TRY(ga.run(a.data, full_nx, n, cent, fin, nullptr, s));
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
    KM_TRY(hipMemcpy(st, ga.stats, 16, hipMemcpyDeviceToHost));
    *a.objective = best_obj;
    if (a.stats) { a.stats[0] = st[0]; a.stats[1] = st_reseed; a.stats[2] = st_draws; a.stats[3] = st[1]; }
    return RBQ_OK;
}

} // namespace rbq
