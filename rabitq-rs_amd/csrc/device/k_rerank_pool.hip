// k_rerank_pool.hip — the pooled rerank (option rerank_pool): the search has run at top_k := pool and left
// every query's pool (ids by ascending estimate, count); this kernel scores each pooled id exactly against its raw vector,
// orders the pool by (exact score, rank in the pool) and writes the best top_k.  gfx950 only.  k_rerank (relayout.hpp) stays
// the kernel of the unpooled rerank; what this one returns for pool <= 1024 is the head of k_rerank's result at top_k := pool.
//
//   k_rerank_pool<IP, RAW>   one workgroup (4 waves) per query.  RAW: the element the raw rows are kept in (kRawF32, or kRawF16 /
//     kRawBf16: rp_score16, DESIGN.md section 28 — a 16-bit element is widened exactly and enters the same chains); what
//     follows describes the f32 rows.
//     S  the exact score, the bits of canon_l2 / canon_dot (kernels.hpp): rp_score_row of rerank_score.hpp, the one copy of the
//        scorer, which the exact range scan (range.hpp) calls too.  Eight lanes serve one candidate, lane j of the eight
//        owns accumulator j: a wave scores 8 candidates at a time, the workgroup 32.  The raw row is NOT read the way the
//        accumulators consume it (lane j element 8 m + j: 4 bytes per lane, 32 bytes per candidate and load): each lane loads 16
//        bytes, the eight lanes one contiguous 128-byte span of the row, kRpSpans spans per step and the next step's already in
//        flight; then four lane permutes per
//        span hand every lane its four elements (round t: lane j receives chunk m = (t + j) & 3 from lane 2 m + (j >> 2), which
//        published component ((lane >> 1) - t) & 3 — so every source lane serves four different readers one component each),
//        and the lane adds them to its chain in the order m = 0 .. 3.  Each accumulator's chain is therefore the sequential
//        chain of the serial loop; the sum -0.0 + acc[0] + ... + acc[7] and the scalar tail dim & ~7 .. dim follow in their
//        order on every lane of the eight.  d * d and + stay two operations (contraction is off for this unit).
//        Rows start 4 dim bytes apart, so a span is 4-byte aligned only: the 16-byte loads are issued as such (global loads of
//        this target need dword alignment, not more).  A span that does not lie wholly inside the row's main part is not read
//        (the row's first 16 bytes stand in, unused), so nothing past raw + n_raw * dim is read.  id >= n_raw scores the NaN
//        0x7fc00000.
//     O  bitonic sort of the keys (ordered score << 32) | rank in LDS — O(c log^2 c) compare-exchanges spread over 256 lanes,
//        78 barriers at 4096 entries — then the first min(top_k, c) entries fetch their ids from the pool; the rest is padded.
// Dynamic LDS: query[dim rounded up to 2] f32 | key[np2(pool)] u64.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

#include "rerank_score.hpp" // (after the pragma: the scorer's sums are unfused)

namespace rbq {

template <bool IP, int RAW>
__global__ __launch_bounds__(kThreads) void k_rerank_pool(RerankPoolParams P) {
    extern __shared__ __align__(16) unsigned char smraw[];
    float* sq = reinterpret_cast<float*>(smraw);                                                    // [dim]
    unsigned long long* key = reinterpret_cast<unsigned long long*>(sq + ((P.dim + 1u) & ~1u));     // [np2]
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t dim = P.dim;
    const uint32_t cnt = min(P.pool_counts[q], P.pool);
    uint32_t np2 = 1;
    while (np2 < cnt) np2 <<= 1; // <= np2(pool), what the launch sized the LDS for
    const uint64_t* pid = P.pool_ids + (size_t)q * P.pool;
    copy_query_widened<kThreads>(sq, P.queries, P.query_dtype, (size_t)q * dim, dim, tid);
    for (uint32_t i = cnt + tid; i < np2; i += kThreads) key[i] = ~0ull; // (above every real key: those carry a rank < 4096)
    __syncthreads();

    // ---- S: eight lanes per candidate, wave-uniform trip counts (a group without a candidate writes nothing)
    const uint32_t j = lane & 7u, grp = lane >> 3, base = lane & ~7u;
    for (uint32_t r0 = wave * 8u; r0 < cnt; r0 += (kThreads / 64u) * 8u) {
        const uint32_t r = r0 + grp;
        const bool have = r < cnt;
        const uint64_t id = have ? pid[r] : ~0ull;
        const bool act = have && id < P.n_raw;
        const float sum = rp_score_row<IP, RAW>(P.raw, id, act, sq, dim, j, base, P.raw_by_element != 0u); // (no candidate, or no raw row: row 0, read and discarded)
        if (have && j == 0u) {
            int32_t k = total_key(act ? sum : __int_as_float(0x7fc00000));
            if (IP) k = ~k;
            key[r] = ((unsigned long long)((uint32_t)k ^ 0x80000000u) << 32) | r;
        }
    }

    // ---- O: ascending bitonic sort of np2 keys (distinct: they carry the rank)
    for (uint32_t size = 2; size <= np2; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (uint32_t i = tid; i < (np2 >> 1); i += kThreads) {
                const uint32_t lo = ((i & ~(stride - 1u)) << 1) | (i & (stride - 1u)), hi = lo | stride;
                const bool up = (lo & size) == 0u;
                const unsigned long long a = key[lo], b = key[hi];
                if ((a > b) == up) { key[lo] = b; key[hi] = a; }
            }
        }
    __syncthreads();
    const uint32_t n_out = min(cnt, P.top_k);
    for (uint32_t i = tid; i < P.top_k; i += kThreads) {
        uint64_t id = ~0ull;
        float sc = __int_as_float(0x7fc00000);
        if (i < n_out) {
            const unsigned long long kk = key[i];
            int32_t k = (int32_t)((uint32_t)(kk >> 32) ^ 0x80000000u);
            if (IP) k = ~k;
            id = pid[(uint32_t)kk];
            sc = key_to_float(k);
        }
        P.out_ids[(size_t)q * P.top_k + i] = id;
        P.out_scores[(size_t)q * P.top_k + i] = sc;
    }
    if (tid == 0) P.out_counts[q] = n_out;
}

namespace {
uint32_t rp_np2(uint32_t n) {
    uint32_t p = 1;
    while (p < n) p <<= 1;
    return p;
}
} // namespace

size_t rerank_pool_lds_bytes(uint32_t dim, uint32_t pool) { return (size_t)((dim + 1u) & ~1u) * 4 + (size_t)rp_np2(pool) * 8; }

namespace {
template <bool IP, int RAW>
hipError_t launch_rp(const RerankPoolParams& P, size_t lds, int device, hipStream_t s) {
    static LdsAttrCache attr;
    const hipError_t e = attr.ensure(reinterpret_cast<const void*>(&k_rerank_pool<IP, RAW>), lds, device);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_rerank_pool<IP, RAW>), dim3(P.nq), dim3(kThreads), lds, s, P);
    return hipGetLastError();
}
template <int RAW>
hipError_t launch_rp(const RerankPoolParams& P, size_t lds, int device, hipStream_t s) {
    return P.metric == 1u ? launch_rp<true, RAW>(P, lds, device, s) : launch_rp<false, RAW>(P, lds, device, s);
}
} // namespace

hipError_t launch_rerank_pool(const RerankPoolParams& P0, int device, hipStream_t s) {
    RerankPoolParams P = P0;
    if (P.nq == 0u || P.dim == 0u || P.n_raw == 0u || P.top_k == 0u || P.pool <= P.top_k || P.pool > kRerankPoolMax) return hipErrorInvalidValue;
    const size_t lds = rerank_pool_lds_bytes(P.dim, P.pool);
    if (lds > kLdsPerWorkgroupMax) return hipErrorInvalidValue;
    // 16-byte loads go to 4-byte aligned addresses only: 16-bit rows all start on one exactly when the base does and dim is even;
    // otherwise the kernel loads element by element (the slow path; callers who care pad dim to even)
    P.raw_by_element = P.raw_dtype != kRawF32 && ((P.dim & 1u) != 0u || (reinterpret_cast<uintptr_t>(P.raw) & 3u) != 0u) ? 1u : 0u;
    if (P.raw_dtype == kRawF32) return launch_rp<kRawF32>(P, lds, device, s);
    if (P.raw_dtype == kRawF16) return launch_rp<kRawF16>(P, lds, device, s);
    if (P.raw_dtype == kRawBf16) return launch_rp<kRawBf16>(P, lds, device, s);
    return hipErrorInvalidValue;
}

} // namespace rbq
