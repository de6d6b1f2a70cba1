// k_mstg_rerank.hip — the exact rerank of the MSTG candidate pool (option mstg_rerank on rbq_mstg_search_refined_batch*; DESIGN.md
// section 35): the binary scan has run at top_k := pool over the identity slot map, exactly as for the refined search (section 19);
// this kernel reduces the pool to one entry per id, scores every distinct id exactly against its raw row, orders the entries by
// (distance, rank) and writes the best top_k.  The stored ex codes are not read.  gfx950 only.
//
//   k_mstg_rerank<IP, RAW>   one workgroup (4 waves) per query.  RAW: the element type of the raw rows (kRawF32 / kRawF16 / kRawBf16).
//     P  the pool: one lane per entry finds the entry's list among the query's ProbeInfo rows (mp_find_list) and, after a barrier,
//        its rank among equal estimates (mp_rank) — mstg_pool.hpp, the copy k_mstg_refine uses.  Then the id, ids[slot]; an entry
//        of no selected list or with id >= n_raw gets the dropped mark.
//     D  bitonic sort of (id, rank); the head of every id run (the smallest rank) survives.  A workgroup prefix sum over the
//        per-thread head counts (every thread owns a contiguous piece of the sorted array) compacts the survivors' positions into
//        a dense list, so the scoring loop has a wave-uniform trip count and no group of eight lanes idles on a duplicate.
//     S  eight lanes per survivor, 32 survivors per round: rp_score_row (rerank_score.hpp: the bits of canon_l2 / canon_dot) over
//        the query widened into LDS.  The reported value is a distance: canon_l2, or -canon_dot.  A non-finite value drops the entry.
//     O  bitonic sort of (distance key << 32 | rank << 12 | place in the dense list); the key orders by value, -0.0 and +0.0 share
//        one, so rank decides between them.  The first top_k entries are written with the scorer's own bits; the rest is padded.
// Dynamic LDS: query[dim rounded up to 2] f32 | k1[np2(pool)] u64 | k2[np2(pool)] u64 | aux[np2(pool)] u32 | 8 u32.
//   aux: P the place j of the entry's list; D, S the dense list (positions in the sorted array); S, O the reported distances.
#include <hip/hip_runtime.h>

#include "rbq_mstg.h"
#include "launch.hpp"
#include "kernels.hpp"
#include "mstg_pool.hpp"

#pragma clang fp contract(off)

#include "rerank_score.hpp" // (after the pragma: the scorer's sums are unfused)

namespace rbq {

static_assert(kMrPoolMax <= 4096, "the order key holds the rank and the dense place in 12 bits each");

template <bool IP, int RAW>
__global__ __launch_bounds__(kThreads) void k_mstg_rerank(MstgRerankParams P) {
    extern __shared__ __align__(16) unsigned char smraw[];
    float* sq = reinterpret_cast<float*>(smraw);                                                // [dim]
    unsigned long long* k1 = reinterpret_cast<unsigned long long*>(sq + ((P.dim + 1u) & ~1u)); // P: the slot; D on: the id
    unsigned long long* k2 = k1 + P.pool_np2;                                                   // P, D: the rank; S, O: the order key
    uint32_t* aux = reinterpret_cast<uint32_t*>(k2 + P.pool_np2);
    uint32_t* s_wsum = aux + P.pool_np2; // [4] head counts of the waves
    uint32_t* s_fin = s_wsum + 4;        // finite survivors
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t dim = P.dim;
    const uint32_t cnt = min(P.pool_counts[q], P.pool);
    uint32_t np2 = 1;
    while (np2 < cnt) np2 <<= 1; // <= P.pool_np2
    const uint32_t lc = min(P.list_counts[q], P.probe_stride);
    const ProbeInfo* probe = P.probe + (size_t)q * P.probe_stride;
    const uint64_t* pslots = P.pool_slots + (size_t)q * P.pool;
    const float* pest = P.pool_scores + (size_t)q * P.pool;
    copy_query_widened<kThreads>(sq, P.queries, P.query_dtype, (size_t)q * dim, dim, tid);
    if (tid == 0) *s_fin = 0u;

    // ---- P: one lane per entry
    for (uint32_t r = tid; r < np2; r += kThreads) {
        const unsigned long long slot = r < cnt ? pslots[r] : kMrDropped;
        float g_add;
        aux[r] = mp_find_list(P.blk_list, probe, lc, slot, P.n_slots, &g_add);
        k1[r] = slot;
    }
    __syncthreads();
    for (uint32_t r = tid; r < np2; r += kThreads)
        k2[r] = r < cnt ? mp_rank(pest, cnt, r, [&](uint32_t i) { return aux[i]; }, [&](uint32_t i) { return (uint32_t)k1[i]; }) : kMrDropped;
    __syncthreads();
    for (uint32_t r = tid; r < np2; r += kThreads) {
        unsigned long long id = kMrDropped;
        if (aux[r] != kMpNoList) id = P.ids[k1[r]]; // (a place was found: the slot is below n_slots)
        if (id >= P.n_raw) { id = kMrDropped; k2[r] = kMrDropped; }
        k1[r] = id;
    }

    // ---- D: one entry per id, the survivors' positions dense in aux
    mr_sort<true>(k1, k2, np2, tid);
    const uint32_t piece = np2 > kThreads ? np2 / kThreads : 1u, i0 = tid * piece; // (np2 is a power of two: the pieces tile it)
    uint32_t heads = 0;
    for (uint32_t i = i0; i < i0 + piece && i < np2; ++i)
        heads += k1[i] != kMrDropped && (i == 0u || k1[i] != k1[i - 1u]) ? 1u : 0u;
    uint32_t incl = heads;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o);
        if (lane >= (uint32_t)o) incl += t;
    }
    if (lane == 63u) s_wsum[wave] = incl;
    __syncthreads();
    uint32_t at = incl - heads, n_surv = 0;
    for (uint32_t w = 0; w < kThreads / 64u; ++w) {
        const uint32_t t = s_wsum[w];
        if (w < wave) at += t;
        n_surv += t;
    }
    for (uint32_t i = i0; i < i0 + piece && i < np2; ++i) {
        const bool head = k1[i] != kMrDropped && (i == 0u || k1[i] != k1[i - 1u]);
        if (head) aux[at++] = i;
        else k2[i] = kMrDropped; // (leaves the order; the heads are decided by k1 alone, which nobody writes here)
    }
    __syncthreads();

    // ---- S: eight lanes per survivor, wave-uniform trip counts (a group without a survivor reads row 0 and writes nothing)
    const uint32_t j = lane & 7u, grp = lane >> 3, base = lane & ~7u;
    for (uint32_t p0 = wave * 8u; p0 < n_surv; p0 += (kThreads / 64u) * 8u) {
        const uint32_t p = p0 + grp;
        const bool have = p < n_surv;
        const uint32_t i = have ? aux[p] : 0u;
        const uint64_t id = have ? k1[i] : 0ull;
        const uint32_t rank = (uint32_t)k2[i];
        const float sum = rp_score_row<IP, RAW>(P.raw, id, have, sq, dim, j, base, P.raw_by_element != 0u);
        if (have && j == 0u) {
            const float dist = IP ? -sum : sum;
            if (finite_f(dist)) {
                const float v = dist == 0.0f ? 0.0f : dist; // the key orders by value
                const uint32_t key = (uint32_t)total_key(v) ^ 0x80000000u;
                k2[i] = ((unsigned long long)key << 32) | (rank << 12) | p;
                aux[p] = __float_as_uint(dist);             // (aux[p] was this group's alone to read)
                atomicAdd(s_fin, 1u);
            } else {
                k2[i] = kMrDropped;
            }
        }
    }

    // ---- O: the order of the result
    mr_sort<false>(k1, k2, np2, tid);
    const uint32_t n_out = min(*s_fin, P.top_k);
    for (uint32_t i = tid; i < P.top_k; i += kThreads) {
        uint64_t id = ~0ull;
        float sc = __int_as_float(0x7fc00000);
        if (i < n_out) {
            id = k1[i];
            sc = __uint_as_float(aux[(uint32_t)k2[i] & 0xfffu]);
        }
        P.out_ids[(size_t)q * P.top_k + i] = id;
        P.out_scores[(size_t)q * P.top_k + i] = sc;
    }
    if (tid == 0) P.out_counts[q] = n_out;
}

// Dynamic LDS of one workgroup: the query, 16 bytes of keys and 4 bytes of aux per pool entry (np2), the prefix sums and the count.
// At pool 4096 and dim 2048: 8192 + 81920 + 32 = 90144 bytes.
size_t mstg_rerank_lds_bytes(uint32_t dim, uint32_t pool_np2) { return (size_t)((dim + 1u) & ~1u) * 4 + (size_t)pool_np2 * 20 + 32; }

namespace {
template <bool IP, int RAW>
hipError_t launch_mrr(const MstgRerankParams& P, size_t lds, int device, hipStream_t s) {
    static LdsAttrCache attr;
    const hipError_t e = attr.ensure(reinterpret_cast<const void*>(&k_mstg_rerank<IP, RAW>), lds, device);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_mstg_rerank<IP, RAW>), dim3(P.nq), dim3(kThreads), lds, s, P);
    return hipGetLastError();
}
template <int RAW>
hipError_t launch_mrr(const MstgRerankParams& P, size_t lds, int device, hipStream_t s) {
    return P.metric == 1u ? launch_mrr<true, RAW>(P, lds, device, s) : launch_mrr<false, RAW>(P, lds, device, s);
}
} // namespace

hipError_t launch_mstg_rerank(const MstgRerankParams& P0, int device, hipStream_t s) {
    MstgRerankParams P = P0;
    if (P.nq == 0u || P.dim == 0u || P.n_raw == 0u || !P.raw || P.top_k == 0u || P.top_k > P.pool) return hipErrorInvalidValue;
    if (P.pool_np2 > kMrPoolMax || P.pool > P.pool_np2 || (P.pool_np2 & (P.pool_np2 - 1u)) != 0u) return hipErrorInvalidValue;
    const size_t lds = mstg_rerank_lds_bytes(P.dim, P.pool_np2);
    if (lds > kLdsPerWorkgroupMax) return hipErrorInvalidValue;
    // as launch_rerank_pool: 16-byte loads go to 4-byte aligned addresses only; 16-bit rows all start on one exactly when the base
    // does and dim is even, otherwise the scorer loads element by element
    P.raw_by_element = P.raw_dtype != kRawF32 && ((P.dim & 1u) != 0u || (reinterpret_cast<uintptr_t>(P.raw) & 3u) != 0u) ? 1u : 0u;
    if (P.raw_dtype == kRawF32) return launch_mrr<kRawF32>(P, lds, device, s);
    if (P.raw_dtype == kRawF16) return launch_mrr<kRawF16>(P, lds, device, s);
    if (P.raw_dtype == kRawBf16) return launch_mrr<kRawBf16>(P, lds, device, s);
    return hipErrorInvalidValue;
}

} // namespace rbq
