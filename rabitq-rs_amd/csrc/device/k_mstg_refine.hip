// k_mstg_refine.hip — the refined MSTG search (include/rbq_mstg.h, rbq_mstg_search_refined_batch*): the
// candidate pool of the binary scan is re-scored with the stored ex codes, reduced to one entry per id and cut to top_k.
// gfx950 only.  The scan kernels are not touched: they run with an identity slot map in place of the id array, so the pool
// arrives as global slot indices (gblock * 32 + lane), rank r of a query = entry r of the binary result.
//
//   k_mr_slot_map / k_mr_blk_list   once per handle: slot_map[s] = s; blk_list[b] = the list that owns block b
//   k_mstg_refine<V>   one workgroup per query, phases over the query's (at most RBQ_MSTG_REFINE_POOL_MAX) candidates:
//     A  one lane per candidate: accu of its sign code from the block record through the query's u8 LUT (in LDS, as the scan
//        reads it), ip = the epilogue's first operation, and the candidate's list among the query's selected lists: its place j
//        in the scan order and g_add, the float k_probes_given wrote for it.
//     R  the rank.  The scan returns the pool ascending by estimate, but its heap leaves the order among EQUAL estimates to the
//        sequence of its pushes and pops; the contract's order there is (list order, vector order), the order of the CPU
//        restatement.  Equal estimates are neighbours, so a candidate's rank is the start of its run of equal values plus the
//        candidates of the run with a smaller (j, slot).  Runs are one candidate long unless estimates tie exactly.
//        (The search for j of phase A and this phase are mp_find_list / mp_rank of mstg_pool.hpp, shared with k_mstg_rerank.hip.)
//     B  the refined distance.  ex_bits > 0: 16 lanes per candidate, as the scan's refine_batch: ex_dot in the handle's numeric
//        variant (ex_dot_units + group16_reduce, or ex_dot_var_rt), then src/ivf.rs:2086-2099 in its operation order.
//        ex_bits == 0: one lane per candidate, the binary estimate in the scan's operation order.
//        Non-finite distances drop the candidate; L2 distances below zero become +0.
//     C  bitonic sort of (id, distance key, rank) in LDS; the first entry of every id run is kept (smallest distance, then
//        smallest rank); the kept entries are sorted by (distance key, rank); the first top_k are written, the rest padded.
//        The distance key orders by value: -0.0 and +0.0 share a key, so rank decides between them.
// Dynamic LDS: lut[4 Dc] | query[ex_qlen] f32 | k1[np2(pool)] u64 | k2[np2(pool)] u64 | dist, j, rank [np2(pool)] 32-bit | kept u32.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rbq.h"
#include "rbq_mstg.h"
#include "launch.hpp"
#include "kernels.hpp"
#include "mstg_pool.hpp"  // mp_find_list, mp_rank, mr_sort: shared with k_mstg_rerank.hip
#include "scan_codes.hpp" // lds_lut_ptr, accumulate_block_rt: the scan's own lookup of one vector's sign code

namespace rbq {

static_assert(RBQ_MSTG_REFINE_POOL_MAX == kMrPoolMax, "rbq_mstg.h and launch.hpp disagree");

__global__ __launch_bounds__(256) void k_mr_slot_map(uint64_t* __restrict__ slot_map, uint64_t n_slots) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n_slots) slot_map[i] = i;
}

__global__ __launch_bounds__(256) void k_mr_blk_list(const uint32_t* __restrict__ list_gb0, const uint32_t* __restrict__ list_n, uint32_t n_lists,
                                                     uint32_t n_blocks, uint32_t* __restrict__ blk_list) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= n_lists) return;
    const uint32_t gb = list_gb0[c], nb = (list_n[c] + 31u) >> 5;
    for (uint32_t b = 0; b < nb; ++b)
        if ((uint64_t)gb + b < n_blocks) blk_list[gb + b] = c;
}

template <int V>
__global__ __launch_bounds__(kThreads) void k_mstg_refine(MstgRefineParams P) {
    extern __shared__ __align__(16) unsigned char smraw[];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t D = P.D, Dc = P.Dc, ex_bits = P.ex_bits;
    const uint32_t qlen = ex_qlen(D, ex_bits), nunits = ex_w4(D, ex_bits);
    const size_t exb = ex_bytes_dev(D, ex_bits), stride = (size_t)Dc * 4 + 384;
    uint8_t* s_lut = smraw;
    float* s_q = reinterpret_cast<float*>(smraw + (size_t)Dc * 4);
    unsigned long long* k1 = reinterpret_cast<unsigned long long*>(s_q + qlen); // A, B: the slot; C: the id
    unsigned long long* k2 = k1 + P.pool_np2;                                   // A, B: g_add | ip; C: distance key | rank
    float* s_d = reinterpret_cast<float*>(k2 + P.pool_np2);                     // [rank] the reported distance
    uint32_t* s_j = reinterpret_cast<uint32_t*>(s_d + P.pool_np2);              // [r] place of the candidate's list in the scan order
    uint32_t* s_rank = s_j + P.pool_np2;                                        // [r] the candidate's rank
    uint32_t* s_kept = s_rank + P.pool_np2;
    const lds_lut_ptr lut = (lds_lut_ptr)(__attribute__((address_space(3))) unsigned char*)smraw;

    const uint32_t cnt = min(P.pool_counts[q], P.pool);
    uint32_t np2 = 1;
    while (np2 < cnt) np2 <<= 1; // <= P.pool_np2
    const uint32_t lc = min(P.list_counts[q], P.probe_stride);
    const ProbeInfo* probe = P.probe + (size_t)q * P.probe_stride;
    const uint64_t* pslots = P.pool_slots + (size_t)q * P.pool;
    const float* pest = P.pool_scores + (size_t)q * P.pool;
    {
        const uint4* src = reinterpret_cast<const uint4*>(P.lut + (size_t)q * Dc * 4);
        uint4* dst = reinterpret_cast<uint4*>(s_lut);
        for (uint32_t i = tid; i < Dc / 4; i += kThreads) dst[i] = src[i];
        const float* rs = P.rot + (size_t)q * D;
        for (uint32_t i = tid; i < qlen; i += kThreads) s_q[i] = i < D ? rs[i] : 0.0f; // (padded code slots are 0: 0 * q + s == s)
        if (tid == 0) *s_kept = 0u;
    }
    const QueryConsts qc = P.consts[q];
    __syncthreads();

    // the candidate at pool position r is final: its id, key and distance, or the dropped mark
    auto finish = [&](uint32_t r, uint32_t slot, float dist) {
        if (!finite_f(dist)) { k1[r] = kMrDropped; k2[r] = kMrDropped; return; }
        if (P.metric == 0) dist = dist > 0.0f ? dist : 0.0f; // distance.max(0.0); -0.0 becomes +0.0
        const uint32_t rank = s_rank[r];
        s_d[rank] = dist;
        const float v = dist == 0.0f ? 0.0f : dist;          // the key orders by value
        const uint32_t key = (uint32_t)total_key(v) ^ 0x80000000u;
        k1[r] = P.ids[slot];
        k2[r] = ((unsigned long long)key << 32) | rank;
    };

    // ---- A: one lane per candidate
    for (uint32_t r = tid; r < np2; r += kThreads) {
        const unsigned long long slot = r < cnt ? pslots[r] : kMrDropped;
        float g_add;
        const uint32_t jfound = mp_find_list(P.blk_list, probe, lc, slot, P.n_slots, &g_add);
        const uint32_t gblock = jfound != kMpNoList ? (uint32_t)(slot >> 5) : 0u, l32 = (uint32_t)slot & 31u;
        s_j[r] = jfound;
        // (a slot out of range or a block of no selected list cannot come out of the scan: such an entry would be dropped)
        if (jfound == kMpNoList) { k1[r] = kMrDropped; k2[r] = kMrDropped; continue; }
        const uint8_t* blk = P.blocks + (size_t)gblock * stride;
        const uint32_t accu = accumulate_block_rt(blk, lut, l32, Dc) & 0xffffu;
        const float ip = epi_ip(qc.delta, (float)accu, qc.sum_vl, V == kVarPortable);
        k1[r] = slot;
        k2[r] = ((unsigned long long)__float_as_uint(g_add) << 32) | __float_as_uint(ip);
    }
    __syncthreads();
    // ---- R: ranks among equal estimates by (list order, vector order)
    for (uint32_t r = tid; r < cnt; r += kThreads) {
        s_rank[r] = mp_rank(pest, cnt, r, [&](uint32_t i) { return s_j[i]; }, [&](uint32_t i) { return (uint32_t)k1[i]; });
    }
    __syncthreads();
    // ---- B: the refined distance
    if (ex_bits == 0) { // the binary estimate, in the scan's operation order
        for (uint32_t r = tid; r < cnt; r += kThreads) {
            const unsigned long long gi = k2[r];
            if (gi == kMrDropped) continue;
            const uint32_t slot = (uint32_t)k1[r];
            const float* fac = reinterpret_cast<const float*>(P.blocks + (size_t)(slot >> 5) * stride + (size_t)Dc * 4);
            const float ip = __uint_as_float((uint32_t)gi), g_add = __uint_as_float((uint32_t)(gi >> 32));
            const float tt = ip + qc.k1x;
            const float rsc = fac[32 + (slot & 31u)] * tt;
            float est = fac[slot & 31u] + g_add;
            est = est + rsc;
            finish(r, slot, est);
        }
    } else { // 16 lanes per candidate (wave-uniform trip count; a group without a candidate evaluates slot 0 and writes nothing)
        const uint32_t grp = tid >> 4, gl = tid & 15u;
        for (uint32_t r0 = 0; r0 < cnt; r0 += kThreads / 16) {
            const uint32_t r = r0 + grp;
            const bool act = r < cnt && k2[r < cnt ? r : 0u] != kMrDropped;
            const uint32_t slot = act ? (uint32_t)k1[r] : 0u;
            const unsigned long long gi = act ? k2[r] : 0ull;
            const uint8_t* ex = P.ex_codes + (size_t)slot * exb;
            const float fa = P.f_add_ex[slot], fr = P.f_rescale_ex[slot];
            float sacc;
            if constexpr (V != kVarAvx512) {
                sacc = ex_dot_var_rt<V>(ex, s_q, gl, nunits, D / 16, ex_bits); // (already the group's sum)
            } else {
                sacc = ex_bits == 6 ? ex_dot_units<6>(ex, s_q, gl, nunits) : ex_dot_units<2>(ex, s_q, gl, nunits);
                sacc = group16_reduce(sacc);
            }
            if (gl == 0 && act) {
                const float ip = __uint_as_float((uint32_t)gi), g_add = __uint_as_float((uint32_t)(gi >> 32));
                float tt2 = qc.scale * ip;
                tt2 = tt2 + sacc;
                tt2 = tt2 + qc.kbx;
                const float a = fa + g_add;
                const float m = fr * tt2;
                finish(r, slot, a + m);
            }
        }
    }
    // ---- C: one entry per id, then the order of the result
    mr_sort<true>(k1, k2, np2, tid);
    uint32_t flags = 0; // bit j: entry tid + j * kThreads opens an id run (np2 <= 4096: at most 16 entries per thread)
    for (uint32_t i = tid, j = 0; i < np2; i += kThreads, ++j)
        if (k2[i] != kMrDropped && (i == 0u || k1[i] != k1[i - 1u])) flags |= 1u << j;
    __syncthreads();
    for (uint32_t i = tid, j = 0; i < np2; i += kThreads, ++j)
        if (!((flags >> j) & 1u)) k2[i] = kMrDropped;
    if (flags) atomicAdd(s_kept, (uint32_t)__popc(flags));
    mr_sort<false>(k1, k2, np2, tid);
    const uint32_t n_out = min(*s_kept, P.top_k);
    for (uint32_t i = tid; i < P.top_k; i += kThreads) {
        uint64_t id = ~0ull;
        float sc = __int_as_float(0x7fc00000);
        if (i < n_out) {
            id = k1[i];
            sc = s_d[(uint32_t)k2[i]];
        }
        P.out_ids[(size_t)q * P.top_k + i] = id;
        P.out_scores[(size_t)q * P.top_k + i] = sc;
    }
    if (tid == 0) P.out_counts[q] = n_out;
}

size_t mstg_refine_lds_bytes(uint32_t D, uint32_t Dc, uint32_t ex_bits, uint32_t pool_np2) {
    return (size_t)Dc * 4 + (size_t)ex_qlen(D, ex_bits) * 4 + (size_t)pool_np2 * 28 + 16;
}

hipError_t launch_mstg_refine_maps(const uint32_t* list_gb0, const uint32_t* list_n, uint32_t n_lists, uint32_t n_blocks, uint64_t* slot_map,
                                   uint32_t* blk_list, hipStream_t s) {
    const uint64_t n_slots = (uint64_t)n_blocks * 32u;
    hipError_t e = hipMemsetAsync(blk_list, 0xff, (size_t)n_blocks * 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mr_slot_map, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, s, slot_map, n_slots);
    hipLaunchKernelGGL(k_mr_blk_list, dim3((n_lists + 255u) / 256u), dim3(256), 0, s, list_gb0, list_n, n_lists, n_blocks, blk_list);
    return hipGetLastError();
}

namespace {
template <int V>
hipError_t launch_refine_v(const MstgRefineParams& P, int device, hipStream_t s) {
    static LdsAttrCache attr;
    const size_t lds = mstg_refine_lds_bytes(P.D, P.Dc, P.ex_bits, P.pool_np2);
    hipError_t e = attr.ensure(reinterpret_cast<const void*>(&k_mstg_refine<V>), lds, device);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_mstg_refine<V>), dim3(P.nq), dim3(kThreads), lds, s, P);
    return hipGetLastError();
}
} // namespace

hipError_t launch_mstg_refine(const MstgRefineParams& P, int device, hipStream_t s) {
    if (P.pool_np2 > kMrPoolMax || P.pool > P.pool_np2 || (P.pool_np2 & (P.pool_np2 - 1u)) != 0u || P.nq == 0u) return hipErrorInvalidValue;
    if (mstg_refine_lds_bytes(P.D, P.Dc, P.ex_bits, P.pool_np2) > kLdsPerWorkgroupMax) return hipErrorInvalidValue;
    if (P.numeric_variant == (uint32_t)kVarAvx2) return launch_refine_v<kVarAvx2>(P, device, s);
    if (P.numeric_variant == (uint32_t)kVarPortable) return launch_refine_v<kVarPortable>(P, device, s);
    return launch_refine_v<kVarAvx512>(P, device, s);
}

} // namespace rbq
