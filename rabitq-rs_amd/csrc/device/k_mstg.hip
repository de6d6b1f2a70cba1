// k_mstg.hip — MSTG closure assignment on the device: ClosureAssigner::assign (reference src/mstg/closure.rs:24-107) of every
// row, bit for bit the CPU restatement rbq_build_closure_assign (csrc/host/rbq_build.cpp).  gfx950 only.
//
// A chunk of R rows at a time (no n x k score matrix), m = min(max_replicas, k):
//   launch_approx_dots  (k_gemm_shortlist.hip) the chunk's rows as split-bf16 hi / lo images, zero-padded to Dp = dim rounded up
//                   to 32, then dA(x, c) by the ranking GEMM's inner-product form (k_rank_bf16_db, rank_mfma.hpp)
//   k_cl_scan       per row: A = max(0, fmaf(-2, dA, nx + nc)); T = the m-th smallest of the 64 lanes' minima of A (m distinct
//                   centroids have A <= T); shortlist {c : A(c) <= T + 2 eps} in centroid order; over kShortlist entries (or
//                   norms near overflow): the row is marked for the fallback
//   k_cl_exact      one wavefront per row: canonical l2_distance_sqr of the shortlist (of all k centroids for a marked row: the
//                   fallback, counted, never approximated), 8 lanes per pair, lane g owning accumulator g of the AVX2 order;
//                   the m first entries under (distance, centroid); threshold; RNG rule with the centroid-pair distances
//                   computed on the fly; the output row in the crate's Vec order
// eps bounds |A - C| for the canonical C of math.rs's diff-squared form.  With E = |x - c|^2 exact:
//   |C - E| <= gamma_(dim+18) E, E <= 2 (|x|^2 + |c|^2)                   (one subtraction, one product, at most dim / 8 + 15 additions)
//   |A - E| <= gamma_(dim+2) (|x|^2 + |c|^2)                                (the sequential norms and their sum)
//            + (3.01 * 2^-16 + 6 Dp u)(|x|^2 + |c|^2)                       (2 |dA - P|, rank_mfma.hpp, S <= (|x|^2 + |c|^2) / 2)
//            + 2.1 u (|x|^2 + |c|^2)                                        (the fmaf's rounding; max(., 0) is 1-Lipschitz, E >= 0)
//   eps = ((10 Dp + 64) u + 4 * 2^-16)(nx + max nc)(1 + 2^-6) + 2^-100 (closure_eps, km_common.hpp) covers all of it for
//   Dp <= 16384, the norms' own error, the margin and underflow included.
// Completeness: let c be among the m first of the exact stable order and suppose A(c) > T + 2 eps.  Then C(c) > T + eps, while the
// m centroids with A <= T have C <= T + eps < C(c): m centroids come strictly before c.  So every such c is shortlisted, ties at
// the cut included, and the shortlist's own (distance, centroid) order is the exact order restricted to it.
// k <= kShortlist: no GEMM, every centroid is scored exactly (not a fallback).  Dp > 16384: every row takes the fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rbq.h"
#include "launch.hpp"
#include "kernels.hpp"
#include "km_common.hpp"

namespace rbq {

constexpr uint32_t kClMaxDp = 16384;          // the shortlist's error bound is stated up to this padded dimension
constexpr uint32_t kNone = 0xffffffffu;

// one wavefront per row of the chunk (k > kShortlist >= 64: every lane sees a centroid): T, eps, shortlist or the fallback mark
__global__ __launch_bounds__(256) void k_cl_scan(const float* __restrict__ dots, uint32_t nr, uint32_t k, uint32_t Dp, uint32_t m,
                                                 const float* __restrict__ nx, const float* __restrict__ nc,
                                                 const uint32_t* __restrict__ ncmax_bits, uint32_t* __restrict__ sl,
                                                 uint32_t* __restrict__ sl_n, unsigned long long* __restrict__ stats) {
    const uint32_t lane = threadIdx.x & 63u, row = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (row >= nr) return;
    const float* d = dots + (size_t)row * k;
    const float x2 = nx[row];
    float lmin = INFINITY;
    for (uint32_t c = lane; c < k; c += 64u) lmin = fminf(lmin, km_approx_dist(d, nc, x2, c));
    // the m-th smallest lane minimum (m <= 64): m rounds of a wave minimum over the keys above the last one
    const unsigned long long mine = ((unsigned long long)__float_as_uint(lmin) << 32) | lane;
    unsigned long long last = 0;
    for (uint32_t r = 0; r < m; ++r) last = cl_wave_min(r == 0 || mine > last ? mine : ~0ull);
    const float T = __uint_as_float((uint32_t)(last >> 32));
    const float span = x2 + __uint_as_float(*ncmax_bits);
    bool over = !(span < 1e37f);
    const uint32_t cnt = shortlist_collect(d, nc, x2, k, T + 2.01f * closure_eps(Dp, span), kShortlist, sl + (size_t)row * kShortlist, lane, over);
    if (lane == 0) {
        sl_n[row] = over ? kFallbackMark : cnt;
        if (over) atomicAdd(&stats[0], 1ull);
        else atomicMax(&stats[1], (unsigned long long)cnt);
    }
}

// one wavefront per row.  sl_n == null: every centroid is an entry (k <= kShortlist).  Entries: the row's shortlist, or all k
// centroids for a marked row, whose distances then go to the row's scores in `dots` (no longer needed) instead of the LDS.
__global__ __launch_bounds__(256) void k_cl_exact(const float* __restrict__ x, uint32_t nr, uint32_t dim, const float* __restrict__ cent,
                                                  uint32_t k, const uint32_t* __restrict__ sl, const uint32_t* __restrict__ sl_n,
                                                  float* dots, float epsilon, uint32_t max_replicas, uint32_t* __restrict__ out_lists,
                                                  uint32_t* __restrict__ out_counts) {
    __shared__ float s_dist[4][kShortlist];
    __shared__ uint32_t s_cc[4][kMstgMaxReplicas];
    __shared__ float s_cd[4][kMstgMaxReplicas];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u, row = blockIdx.x * 4u + w;
    if (row >= nr) return; // (the whole wave: the kernel has no workgroup barrier)
    const float* xr = x + (size_t)row * dim;
    const uint32_t n = sl_n ? sl_n[row] : k;
    const bool all = !sl_n || n == kFallbackMark;
    const uint32_t cnt = all ? k : n;
    const uint32_t* srow = all ? nullptr : sl + (size_t)row * kShortlist;
    float* dist = cnt <= kShortlist ? s_dist[w] : dots + (size_t)row * k;
    // canonical distances, 8 entries at a time
    for (uint32_t e0 = 0; e0 < cnt; e0 += 8u) {
        const uint32_t e = e0 + (lane >> 3);
        const bool act = e < cnt;
        const uint32_t c = act ? (all ? e : srow[e]) : 0u;
        const float v = cl_canon8(xr, cent + (size_t)c * dim, dim, lane);
        if (act && (lane & 7u) == 0u) dist[e] = v;
    }
    __threadfence_block(); // (written by this wave: the stores are complete before the loads below)
    // the m first entries under (distance, entry): entries ascend with the centroid index, distances are non-negative and no NaN
    const uint32_t m = min(max_replicas, cnt);
    unsigned long long last = 0;
    for (uint32_t r = 0; r < m; ++r) {
        unsigned long long best = ~0ull;
        for (uint32_t e = lane; e < cnt; e += 64u) {
            const unsigned long long key = ((unsigned long long)__float_as_uint(dist[e]) << 32) | e;
            if ((r == 0 || key > last) && key < best) best = key;
        }
        last = cl_wave_min(best);
        if (lane == 0) {
            const uint32_t e = (uint32_t)last;
            s_cc[w][r] = all ? e : srow[e];
            s_cd[w][r] = __uint_as_float((uint32_t)(last >> 32));
        }
    }
    __threadfence_block();
    // closest * (1.0 + epsilon): the sum is rounded first.  The candidates are a prefix of the sorted entries.
    const float one_eps = 1.0f + epsilon;
    const float threshold = s_cd[w][0] * one_eps;
    const uint32_t ncand = (uint32_t)__popcll(__ballot(lane < m && s_cd[w][lane] <= threshold));
    // RNG rule: candidate j goes when a kept candidate s has dist(j, v) > dist(s, j); the closest is always kept
    unsigned long long kept = 1ull;
    for (uint32_t j = 1; j < ncand; ++j) {
        const float dj = s_cd[w][j];
        const float* cj = cent + (size_t)s_cc[w][j] * dim;
        bool drop = false;
        for (uint32_t s0 = 0; s0 < j && !drop; s0 += 8u) {
            if (((kept >> s0) & 0xffull) == 0) continue;
            const uint32_t s = s0 + (lane >> 3);
            const bool act = s < j && ((kept >> s) & 1ull);
            const float* cs = act ? cent + (size_t)s_cc[w][s] * dim : cj;
            const float pd = cl_canon8(cs, cj, dim, lane);
            drop = __any(act && dj > pd);
        }
        if (!drop) kept |= 1ull << j;
    }
    const uint32_t nk = (uint32_t)__popcll(kept);
    uint32_t* o = out_lists + (size_t)row * max_replicas;
    if (lane < ncand && ((kept >> lane) & 1ull)) o[__popcll(kept & ((1ull << lane) - 1ull))] = s_cc[w][lane];
    if (lane >= nk && lane < max_replicas) o[lane] = kNone;
    if (lane == 0) out_counts[row] = nk;
}

__global__ __launch_bounds__(256) void k_cl_expand(const uint32_t* __restrict__ lists, const uint32_t* __restrict__ counts,
                                                   const uint32_t* __restrict__ off, uint64_t n, uint32_t max_replicas,
                                                   uint32_t* __restrict__ pair_list, uint32_t* __restrict__ pair_vec) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = counts[i], o = off[i];
    for (uint32_t j = 0; j < c; ++j) {
        pair_list[o + j] = lists[i * max_replicas + j];
        pair_vec[o + j] = (uint32_t)i;
    }
}

hipError_t launch_closure_expand(const uint32_t* lists, const uint32_t* counts, const uint32_t* off, uint64_t n, uint32_t max_replicas,
                                 uint32_t* pair_list, uint32_t* pair_vec, hipStream_t s) {
    hipLaunchKernelGGL(k_cl_expand, dim3(grid_of(n, 256)), dim3(256), 0, s, lists, counts, off, n, max_replicas, pair_list, pair_vec);
    return hipGetLastError();
}

// Bytes of the per-chunk workspace per row: the GEMM front's (or the scores alone), a host caller's staged row, the output row.
static uint64_t cl_chunk_rows(const ClosureArgs& a, uint32_t Dp, bool gemm, bool ident) {
    uint64_t per_row = 4ull * a.max_replicas + 8;
    if (gemm) per_row += gemm_shortlist_row_bytes(a.k, Dp, kShortlist);
    else if (!ident) per_row += 4 * a.k;
    if (!a.data_on_device) per_row += 4ull * a.dim;
    uint64_t r = std::max<uint64_t>(kKmeansChunkBytes / per_row, 1);
    if (a.max_chunk_rows) r = std::min(r, a.max_chunk_rows);
    return std::min<uint64_t>(r, a.n);
}

int closure_device(const ClosureArgs& a, int device, std::string& detail) {
    const uint64_t n = a.n, k = a.k;
    const uint32_t dim = a.dim, Dp = km_dp(dim), M = a.max_replicas;
    const bool ident = k <= kShortlist, gemm = !ident && Dp <= kClMaxDp, tap = a.tap_sl != nullptr;
    const uint64_t R = cl_chunk_rows(a, Dp, gemm, ident), Rp = (R + 127) / 128 * 128; // (the GEMM's row tiles)
    hipStream_t s = 0;
    KmTemp t;
    float *cent = nullptr, *d_in = nullptr, *nx = nullptr, *dots = nullptr;
    uint32_t *flag = nullptr, *sl = nullptr, *sl_n = nullptr, *o_lists = nullptr, *o_counts = nullptr;
    uint16_t *xh = nullptr, *xl = nullptr;
    CentView cv{(uint32_t)k, dim, Dp, nullptr, nullptr, nullptr, nullptr};
    unsigned long long* stats = nullptr;
    KM_TRY(t.alloc(&flag, 1));
    KM_TRY(t.alloc(&stats, 2));
    KM_TRY(hipMemsetAsync(stats, 0, 16, s));
    if (a.cent_on_device) cent = const_cast<float*>(a.centroids);
    else {
        KM_TRY(t.alloc(&cent, k * dim));
        KM_TRY(hipMemcpy(cent, a.centroids, k * dim * 4, hipMemcpyHostToDevice));
    }
    // finite input only (the crate would panic on a NaN distance): checked before a chunk is scored or any of its rows written
    bool bad = false;
    KM_TRY(nonfinite_sync(cent, k * dim, flag, s, &bad));
    if (bad) { detail = "closure assignment input must be finite"; return RBQ_INVALID_CONFIG; }
    if (!a.data_on_device) KM_TRY(t.alloc(&d_in, R * dim));
    if (!ident) {
        KM_TRY(t.alloc(&dots, Rp * k));
        KM_TRY(t.alloc(&sl, R * kShortlist));
        KM_TRY(t.alloc(&sl_n, R));
        KM_TRY(hipMemsetAsync(sl_n, 0xff, R * 4, s)); // (without the GEMM every row stays marked)
    }
    if (gemm) {
        KM_TRY(t.alloc(&nx, R));
        KM_TRY(t.alloc(&cv.nc, k));
        KM_TRY(t.alloc(&cv.ncmax_bits, 1));
        KM_TRY(t.alloc(&xh, Rp * Dp));
        KM_TRY(t.alloc(&xl, Rp * Dp));
        KM_TRY(t.alloc(&cv.hi, k * Dp));
        KM_TRY(t.alloc(&cv.lo, k * Dp));
        KM_TRY(launch_split_centroids(cent, cv, s));
    }
    if (!tap && !a.out_on_device) {
        KM_TRY(t.alloc(&o_lists, R * M));
        KM_TRY(t.alloc(&o_counts, R));
    }
    const uint32_t m = (uint32_t)std::min<uint64_t>(M, k);
    uint64_t marked = 0;
    for (uint64_t r0 = 0; r0 < n; r0 += R) {
        const uint32_t nr = (uint32_t)std::min<uint64_t>(R, n - r0);
        const float* xc = a.data + r0 * dim;
        if (!a.data_on_device) {
            KM_TRY(hipMemcpy(d_in, xc, (size_t)nr * dim * 4, hipMemcpyHostToDevice));
            xc = d_in;
        }
        KM_TRY(nonfinite_sync(xc, (uint64_t)nr * dim, flag, s, &bad));
        if (bad) { detail = "closure assignment input must be finite"; return RBQ_INVALID_CONFIG; }
        if (gemm) {
            KM_TRY(launch_row_norms(xc, nr, dim, nx, s));
            KM_TRY(launch_approx_dots(xc, nr, dim, cv, xh, xl, dots, device, s));
            hipLaunchKernelGGL(k_cl_scan, dim3(grid_of(nr, 4)), dim3(256), 0, s, dots, nr, (uint32_t)k, Dp, m, nx, cv.nc, cv.ncmax_bits, sl, sl_n, stats);
            KM_TRY(hipGetLastError());
        } else if (!ident) {
            marked += nr;
        }
        if (tap) {
            if (ident) {
                for (uint64_t i = r0; i < r0 + nr; ++i) {
                    a.tap_sl_n[i] = (uint32_t)k;
                    for (uint32_t e = 0; e < kShortlist; ++e) a.tap_sl[i * kShortlist + e] = e < k ? e : kNone;
                }
            } else {
                KM_TRY(hipMemcpy(a.tap_sl + r0 * kShortlist, sl, (size_t)nr * kShortlist * 4, hipMemcpyDeviceToHost));
                KM_TRY(hipMemcpy(a.tap_sl_n + r0, sl_n, (size_t)nr * 4, hipMemcpyDeviceToHost));
            }
            continue;
        }
        uint32_t* ol = a.out_on_device ? a.out_lists + r0 * M : o_lists;
        uint32_t* oc = a.out_on_device ? a.out_counts + r0 : o_counts;
        hipLaunchKernelGGL(k_cl_exact, dim3(grid_of(nr, 4)), dim3(256), 0, s, xc, nr, dim, cent, (uint32_t)k, sl, sl_n, dots, a.epsilon, M, ol, oc);
        KM_TRY(hipGetLastError());
        if (!a.out_on_device) {
            KM_TRY(hipMemcpy(a.out_lists + r0 * M, o_lists, (size_t)nr * M * 4, hipMemcpyDeviceToHost));
            KM_TRY(hipMemcpy(a.out_counts + r0, o_counts, (size_t)nr * 4, hipMemcpyDeviceToHost));
        } else if (!a.data_on_device) {
            KM_TRY(hipStreamSynchronize(s)); // the staged rows are reused by the next chunk
        }
    }
    unsigned long long st[2] = {0, 0};
    KM_TRY(hipMemcpy(st, stats, 16, hipMemcpyDeviceToHost));
    if (a.fallbacks) *a.fallbacks = st[0] + marked;
    return RBQ_OK;
}

} // namespace rbq
