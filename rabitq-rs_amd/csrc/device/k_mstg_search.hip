// k_mstg_search.hip — the list selection of MstgIndex::search on the device (include/rbq_mstg.h, "the selection"): the exact
// ef nearest centroids of every query under (bits of the canonical squared distance S, centroid index), cut by dynamic_prune's
// threshold; bit for bit the CPU restatement rbq_build_mstg_select_lists (csrc/host/rbq_build.cpp).  gfx950 only.
//
// A chunk of R queries at a time, ef = min(ef_search, k):
//   launch_row_norms / launch_approx_dots   (k_gemm_shortlist.hip) the front of every GEMM-shortlist path: dA(q, c) for every centroid
//   k_ms_scan    one wavefront per query, no barrier: A = max(0, fmaf(-2, dA, nq + nc)); T = the ef-th smallest A, by a radix
//                select over its bit pattern (four passes of a 256-bin histogram); U = an upper bound of every A a list that
//                survives dynamic_prune can have; shortlist {c : A(c) <= min(T, U) + 2 eps} in centroid order; over kMsCap
//                entries (or norms near overflow / not finite): the query is marked for the fallback and counted
//   k_ms_exact   one workgroup per query: canonical S (canon_pair2, the routine k_probes_given takes g_add from) of the
//                shortlist — of all k centroids for a marked query or when k <= kShortlist — sorted by (bits of S, centroid);
//                the ef first; d = sqrtf(S); thr = d(first) * (1 + pruning_epsilon); the kept prefix, in scan order
// The selected lists then go through k_probes_given and the scan exactly as a caller's own lists do (rbq_posting_scan_batch).
//
// eps is closure_eps (km_common.hpp; derived in k_mstg.hip and DESIGN.md section 15): |A(c) - S(c)| <= eps for finite input with nq + max nc < 1e37.
// Completeness.  B = min(T, U).  A centroid c with A(c) > B + 2 eps has S(c) > B + eps.
//   B = T: the ef centroids with A <= T have S <= T + eps < S(c), so ef centroids come strictly before c: c is not among the ef
//          first, and the shortlist's first ef under (bits, index) are the exact ones.
//   B = U: U >= (min A + eps) ope^2 (1 + 2^-13) + 2^-100 with ope = 1.0f + pruning_epsilon >= 1, and min S <= min A + eps; a kept
//          list has sqrtf(S) <= sqrtf(min S) * ope up to three roundings, so S <= min S * ope^2 (1 + 2^-21) <= U - eps': c is
//          pruned, and so is every centroid behind it (d is monotone in S).  The closest centroid has A <= min A + 2 eps <= B + 2 eps.
// ope < 1, NaN or infinite: U is not used.  A query with a non-finite coordinate has a non-finite norm and falls back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "rbq.h"
#include "rbq_mstg.h"
#include "launch.hpp"
#include "kernels.hpp"
#include "canon_score.hpp"
#include "km_common.hpp"

namespace rbq {

constexpr uint32_t kMsNone = 0xffffffffu;
static_assert(RBQ_MSTG_SHORTLIST == kShortlist && RBQ_MSTG_SEARCH_SHORTLIST == kMsCap, "rbq_mstg.h and the kernels disagree");

// the wave's exclusive prefix sum of v and (in *total) its sum
__device__ __forceinline__ uint32_t ms_wave_excl(uint32_t v, uint32_t lane, uint32_t* total) {
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o);
        if (lane >= (uint32_t)o) inc += t;
    }
    *total = __shfl(inc, 63);
    return inc - v;
}

// one wavefront per query of the chunk (k > kShortlist: the GEMM path).  ef in 1..k.
__global__ __launch_bounds__(256) void k_ms_scan(const float* __restrict__ dots, uint32_t nr, uint32_t k, uint32_t Dp, uint32_t ef,
                                                 float ope, const float* __restrict__ nx, const float* __restrict__ nc,
                                                 const uint32_t* __restrict__ ncmax_bits, uint32_t cent_bad, uint32_t* __restrict__ sl,
                                                 uint32_t* __restrict__ sl_n, unsigned long long* __restrict__ fallbacks) {
    __shared__ uint32_t s_hist[4][256];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u, row = blockIdx.x * 4u + w;
    if (row >= nr) return; // (the whole wave: the kernel has no workgroup barrier)
    const float* d = dots + (size_t)row * k;
    const float x2 = nx[row];
    const float span = x2 + __uint_as_float(*ncmax_bits);
    const float eps = closure_eps(Dp, span);
    bool over = cent_bad != 0u || !(span < 1e37f);
    uint32_t* hist = s_hist[w];
    uint32_t prefix = 0, rank = ef, minb = 0x7f800000u;
    for (int pass = 0; pass < 4 && !over; ++pass) {
        const uint32_t shift = 24u - 8u * (uint32_t)pass;
        for (uint32_t b = lane; b < 256u; b += 64u) hist[b] = 0u;
        __threadfence_block();
        for (uint32_t c = lane; c < k; c += 64u) {
            const uint32_t a = __float_as_uint(km_approx_dist(d, nc, x2, c));
            if (pass == 0) minb = min(minb, a);
            if (pass == 0 || (a >> (shift + 8u)) == (prefix >> (shift + 8u))) atomicAdd(&hist[(a >> shift) & 255u], 1u);
        }
        __threadfence_block();
        // the bin that holds the rank-th smallest of the elements counted: lane l owns bins 4l .. 4l + 3
        const uint32_t h0 = hist[4u * lane], h1 = hist[4u * lane + 1u], h2 = hist[4u * lane + 2u], h3 = hist[4u * lane + 3u];
        uint32_t total;
        const uint32_t before = ms_wave_excl(h0 + h1 + h2 + h3, lane, &total);
        const unsigned long long hit = __ballot(before + h0 + h1 + h2 + h3 >= rank);
        const uint32_t src = (uint32_t)__ffsll((long long)hit) - 1u; // (rank <= total: some lane holds it)
        uint32_t bin = 4u * lane, r = rank - before;
        if (r > h0) { r -= h0; ++bin; if (r > h1) { r -= h1; ++bin; if (r > h2) { r -= h2; ++bin; } } }
        prefix |= (uint32_t)__shfl((int)bin, (int)src) << shift;
        rank = (uint32_t)__shfl((int)r, (int)src);
        __threadfence_block();
    }
    uint32_t cnt = 0;
    if (!over) {
        for (int o = 32; o >= 1; o >>= 1) minb = min(minb, (uint32_t)__shfl_xor((int)minb, o));
        const float T = __uint_as_float(prefix);
        float B = T;
        if (ope >= 1.0f && ope < INFINITY) {
            const float U = fmaf((__uint_as_float(minb) + eps) * ope * ope, 1.0001220703125f, 7.888609052210118e-31f);
            B = fminf(T, U); // (U = inf or NaN after an overflow: fminf keeps T)
        }
        cnt = shortlist_collect(d, nc, x2, k, B + 2.01f * eps, kMsCap, sl + (size_t)row * kMsCap, lane, over);
    }
    if (lane == 0) {
        sl_n[row] = over ? kFallbackMark : cnt;
        if (over) atomicAdd(fallbacks, 1ull);
    }
}

// ascending bitonic sort of keys[0, np2) by the workgroup (np2 a power of two, in LDS or global memory)
__device__ __forceinline__ void ms_sort(unsigned long long* keys, uint32_t np2, uint32_t tid) {
    for (uint32_t size = 2; size <= np2; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (uint32_t i = tid; i < (np2 >> 1); i += kThreads) {
                const uint32_t lo = ((i & ~(stride - 1u)) << 1) | (i & (stride - 1u)), hi = lo | stride;
                const bool up = (lo & size) == 0u;
                const unsigned long long a = keys[lo], b = keys[hi];
                if ((a > b) == up) { keys[lo] = b; keys[hi] = a; }
            }
        }
    __syncthreads();
}

// one workgroup per query.  sl_n == null: every centroid is an entry (k <= kShortlist).  Entries: the query's shortlist, or all
// k centroids for a marked query, whose keys then live in keys_g ([nr][np2(k)] u64; needed when k > kMsCap only).
__global__ __launch_bounds__(kThreads) void k_ms_exact(const float* __restrict__ rot, uint32_t D, const float* __restrict__ cent, uint32_t k,
                                                       const uint32_t* __restrict__ sl, const uint32_t* __restrict__ sl_n,
                                                       unsigned long long* __restrict__ keys_g, uint32_t knp2, uint32_t ef, float ope,
                                                       uint32_t* __restrict__ out_lists, uint32_t* __restrict__ out_counts) {
    __shared__ __align__(16) float s_q[2048];
    __shared__ unsigned long long s_keys[kMsCap];
    __shared__ uint32_t s_flag[2]; // a NaN distance seen; lists kept
    const uint32_t row = blockIdx.x, tid = threadIdx.x, h = tid & 1u, grp = tid >> 1;
    for (uint32_t i = tid; i < D; i += kThreads) s_q[i] = rot[(size_t)row * D + i];
    if (tid < 2u) s_flag[tid] = 0u;
    const uint32_t n = sl_n ? sl_n[row] : k;
    const bool all = !sl_n || n == kFallbackMark;
    const uint32_t cnt = all ? k : n;
    const uint32_t* srow = all ? nullptr : sl + (size_t)row * kMsCap;
    uint32_t np2 = 1;
    while (np2 < cnt) np2 <<= 1;
    unsigned long long* keys = cnt <= kMsCap ? s_keys : keys_g + (size_t)row * knp2;
    __syncthreads();
    for (uint32_t e0 = 0; e0 < np2; e0 += kThreads / 2) { // (uniform trip count: both lanes of a pair take the shuffles together)
        const uint32_t e = e0 + grp;
        const bool act = e < cnt;
        const uint32_t c = act ? (all ? e : srow[e]) : 0u;
        const float s = canon_pair2<0>(s_q, cent + (size_t)c * D, D, h);
        if (h == 0u && e < np2) {
            if (act && s != s) s_flag[0] = 1u;
            keys[e] = act ? ((unsigned long long)__float_as_uint(s) << 32) | c : ~0ull;
        }
    }
    ms_sort(keys, np2, tid);
    const uint32_t take = min(ef, cnt);
    const float s0 = cnt ? __uint_as_float((uint32_t)(keys[0] >> 32)) : 0.0f;
    // closest * (1.0 + pruning_epsilon): the sum is rounded first (ope).  A NaN distance, or a closest one of +inf: nothing.
    const bool none = s_flag[0] != 0u || take == 0u || !(s0 < INFINITY);
    const float threshold = sqrtf(s0) * ope;
    uint32_t mine = 0;
    if (!none)
        for (uint32_t e = tid; e < take; e += kThreads) mine += sqrtf(__uint_as_float((uint32_t)(keys[e] >> 32))) <= threshold ? 1u : 0u;
    if (mine) atomicAdd(&s_flag[1], mine);
    __syncthreads();
    const uint32_t kept = s_flag[1]; // (a prefix: d is monotone in S)
    for (uint32_t e = tid; e < ef; e += kThreads) out_lists[(size_t)row * ef + e] = e < kept ? (uint32_t)keys[e] : kMsNone;
    if (tid == 0u) out_counts[row] = kept;
}

// every query of the chunk is scored against every centroid (the padded dimension is beyond the shortlist's error bound)
__global__ __launch_bounds__(256) void k_ms_mark(uint32_t* __restrict__ sl_n, uint32_t nr, unsigned long long* __restrict__ fallbacks) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < nr) sl_n[i] = kFallbackMark;
    if (i == 0u) atomicAdd(fallbacks, (unsigned long long)nr);
}

__global__ __launch_bounds__(256) void k_ms_fill_none(uint32_t* __restrict__ lists, uint64_t n_lists_words, uint32_t* __restrict__ counts, uint32_t nr) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n_lists_words) lists[i] = kMsNone;
    if (i < nr) counts[i] = 0u;
}

bool mstg_select_gemm(uint64_t k, uint32_t D) { return k > kShortlist && km_dp(D) <= 16384u; }
uint32_t mstg_select_knp2(uint64_t k) {
    if (k <= kMsCap) return 0;
    uint32_t p = 1;
    while (p < k) p <<= 1;
    return p;
}

hipError_t launch_mstg_select(const MstgSelectParams& p, int device, hipStream_t s) {
    const uint32_t D = p.cv.dim, k = p.cv.k, ef = std::min(p.ef_search, k);
    if (ef == 0) { // no list can be selected: counts 0 (the list rows have no slot)
        hipLaunchKernelGGL(k_ms_fill_none, dim3(grid_of(p.nq, 256)), dim3(256), 0, s, p.out_lists, (uint64_t)0, p.out_counts, p.nq);
        return hipGetLastError();
    }
    const float ope = 1.0f + p.pruning_epsilon;
    const bool ident = k <= kShortlist;
    if (!ident && mstg_select_gemm(k, D)) {
        hipError_t e;
        if ((e = launch_row_norms(p.rot, p.nq, D, p.nx, s)) || (e = launch_approx_dots(p.rot, p.nq, D, p.cv, p.q_hi, p.q_lo, p.dots, device, s)))
            return e;
        hipLaunchKernelGGL(k_ms_scan, dim3(grid_of(p.nq, 4)), dim3(256), 0, s, p.dots, p.nq, k, p.cv.Dp, ef, ope, p.nx, p.cv.nc, p.cv.ncmax_bits,
                           p.cent_bad, p.sl, p.sl_n, p.fallbacks);
    } else if (!ident) {
        hipLaunchKernelGGL(k_ms_mark, dim3(grid_of(p.nq, 256)), dim3(256), 0, s, p.sl_n, p.nq, p.fallbacks);
    }
    hipLaunchKernelGGL(k_ms_exact, dim3(p.nq), dim3(kThreads), 0, s, p.rot, D, p.cent, k, p.sl, ident ? nullptr : p.sl_n, p.keys_g,
                       mstg_select_knp2(k), ef, ope, p.out_lists, p.out_counts);
    return hipGetLastError();
}

} // namespace rbq
