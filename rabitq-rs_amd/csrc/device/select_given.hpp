// select_given.hpp — the two selection kernels whose scores are given exactly: k_select (the nprobe best lists of the all-pairs canonical
// ranking k_rank_scores, kept as the exact_rank option and for nprobe beyond the LDS) and k_probes_given (the posting lists an MSTG
// search names).  Both write their streams list by list with the serial writers of select_common.hpp; neither is on a timed path.
// Included by k_query.hip only.
#pragma once
#include "canon_score.hpp"
#include "select_common.hpp"

namespace rbq {

// UNF: the epilogue's first operation is not fused (kVarPortable: block_lbmin)
template <bool UNF = false>
__global__ __launch_bounds__(kThreads) void k_select(const float* __restrict__ scores, uint32_t nlist, uint32_t nprobe,
                                                     uint32_t np2, int metric, const float* __restrict__ rot,
                                                     const float* __restrict__ cent, uint32_t D,
                                                     const uint32_t* __restrict__ list_gb0,
                                                     const uint32_t* __restrict__ list_n,
                                                     ProbeInfo* __restrict__ probe, StreamItem* __restrict__ wl,
                                                     uint64_t wl_stride, uint32_t* __restrict__ nstream,
                                                     unsigned long long* __restrict__ nvec_probed,
                                                     unsigned long long* __restrict__ prof_total,
                                                     const QueryConsts* __restrict__ consts,
                                                     const BlockSummary* __restrict__ bsum, uint64_t* gsel) {
    // gsel != null: the key window [nq][np2] lives in global memory (nprobe beyond what the LDS of one compute unit holds:
    // the reference only clamps nprobe to the number of lists, src/ivf.rs:1791 — slow here, but served)
    extern __shared__ __align__(16) unsigned char smraw[];
    uint64_t* sel = gsel ? gsel + (size_t)blockIdx.x * np2 : reinterpret_cast<uint64_t*>(smraw);
    float* qrot = reinterpret_cast<float*>(smraw + (gsel ? (size_t)0 : (size_t)np2 * 8));
    uint32_t* part = reinterpret_cast<uint32_t*>(qrot + D);
    __shared__ uint32_t hist[256];
    __shared__ uint64_t s_prefix, s_mask;
    __shared__ uint32_t s_k, s_cnt;
    __shared__ unsigned long long s_nvec;
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const float* sc = scores + (size_t)q * nlist;
    for (uint32_t i = tid; i < D; i += kThreads) qrot[i] = rot[(size_t)q * D + i];
    if (tid == 0) { s_prefix = 0; s_mask = 0; s_k = nprobe - 1; s_cnt = 0; s_nvec = 0; }
    __syncthreads();
    // the nprobe-th key; every list when there are no more than nprobe
    const auto key_of = [&](uint32_t i) { return make_key(sc[i], i, metric); };
    const uint64_t kstar = nprobe < nlist ? radix_kth_key(key_of, nlist, tid, hist, &s_prefix, &s_mask, &s_k) : ~0ull;
    for (uint32_t i = tid; i < np2; i += kThreads) sel[i] = ~0ull;
    if (gsel) __threadfence_block();
    __syncthreads();
    for (uint32_t i = tid; i < nlist; i += kThreads) {
        const uint64_t key = key_of(i);
        if (key <= kstar) {
            uint32_t pos = atomicAdd(&s_cnt, 1u);
            if (pos < np2) sel[pos] = key;
        }
    }
    if (gsel) __threadfence_block(); // (global window: the workgroup's own writes are read back by other lanes)
    __syncthreads();
    bitonic_sort_keys(sel, np2, tid, gsel != nullptr);
    // per-probe constants + block counts
    const uint32_t per = (nprobe + kThreads - 1) / kThreads;
    const uint32_t r0 = tid * per, r1 = (r0 + per < nprobe) ? r0 + per : nprobe;
    uint32_t local = 0;
    unsigned long long local_vec = 0;
    for (uint32_t r = r0; r < r1; ++r) {
        const uint32_t cid = (uint32_t)(sel[r] & 0xffffffffu);
        probe[(size_t)q * nprobe + r] = probe_info(metric, sc[cid], metric == 0 ? 0.0f : canon_l2(qrot, cent + (size_t)cid * D, D), cid);
        local += (list_n[cid] + 31u) >> 5;
        local_vec += list_n[cid];
    }
    if (local_vec) atomicAdd(&s_nvec, local_vec);
    uint32_t run;
    uint64_t pos = (uint64_t)q * wl_stride + serial_scan_excl256(local, part, tid, run);
    if (tid == 0) {
        nstream[q] = run;
        nvec_probed[q] = s_nvec; // sum of n_c over the probed lists: the scan's algorithmic work
        if (prof_total) atomicAdd(prof_total + prof_stripe(q), s_nvec);
    }
    const QueryConsts qc = consts[q];
    for (uint32_t r = r0; r < r1; ++r) {
        const uint32_t cid = (uint32_t)(sel[r] & 0xffffffffu);
        const ProbeInfo pi = probe[(size_t)q * nprobe + r]; // written by this thread above
        pos = write_list_blocks(wl, pos, r, list_gb0[cid], list_n[cid], pi, qc, bsum, UNF);
    }
}

// MSTG posting-list scan: the caller supplies each query's posting lists; this emits the
// per-list constants of search_posting_list_fastscan (g_add = l2_distance_sqr(query, centroid) or -dot in
// canonical order, g_error = 0; src/mstg/index.rs:227-231) and the block work list, in the given order.
// dynamic LDS: qrot[D] f32 | part[256] u32.  UNF: as k_select's
template <bool UNF = false>
__global__ __launch_bounds__(kThreads) void k_probes_given(const uint32_t* __restrict__ list_ids,
                                                           const uint32_t* __restrict__ list_counts, uint32_t max_lists,
                                                           uint32_t nlist, int metric, const float* __restrict__ rot,
                                                           const float* __restrict__ cent, uint32_t D,
                                                           const uint32_t* __restrict__ list_gb0,
                                                           const uint32_t* __restrict__ list_n,
                                                           ProbeInfo* __restrict__ probe, StreamItem* __restrict__ wl,
                                                           uint64_t wl_stride, uint32_t* __restrict__ nstream,
                                                           const QueryConsts* __restrict__ consts,
                                                           const BlockSummary* __restrict__ bsum) {
    extern __shared__ __align__(16) unsigned char smraw[];
    float* qrot = reinterpret_cast<float*>(smraw);
    uint32_t* part = reinterpret_cast<uint32_t*>(qrot + D);
    const uint32_t q = blockIdx.x, tid = threadIdx.x, l2 = tid & 1u, grp = tid >> 1;
    for (uint32_t i = tid; i < D; i += kThreads) qrot[i] = rot[(size_t)q * D + i];
    __syncthreads();
    const uint32_t cnt = list_counts[q] < max_lists ? list_counts[q] : max_lists;
    const uint32_t* mine = list_ids + (size_t)q * max_lists;
    for (uint32_t i0 = 0; i0 < cnt; i0 += kThreads / 2) {
        const uint32_t r = i0 + grp;
        if (r < cnt) {
            const uint32_t cid = mine[r];
            float s = 0.0f;
            if (cid < nlist) {
                const float* c = cent + (size_t)cid * D;
                s = metric == 0 ? canon_pair2<0>(qrot, c, D, l2) : canon_pair2<1>(qrot, c, D, l2);
            }
            if (l2 == 0) probe[(size_t)q * max_lists + r] = probe_info_given(metric, s, cid);
        }
    }
    const uint32_t per = (cnt + kThreads - 1) / kThreads;
    const uint32_t r0 = tid * per, r1 = (r0 + per < cnt) ? r0 + per : cnt;
    uint32_t local = 0;
    for (uint32_t r = r0; r < r1; ++r) {
        const uint32_t cid = mine[r];
        if (cid < nlist) local += (list_n[cid] + 31u) >> 5;
    }
    uint32_t run;
    uint64_t pos = (uint64_t)q * wl_stride + serial_scan_excl256(local, part, tid, run);
    if (tid == 0) nstream[q] = run;
    const QueryConsts qcs = consts[q];
    for (uint32_t r = r0; r < r1; ++r) {
        const uint32_t cid = mine[r];
        if (cid >= nlist) continue;
        const ProbeInfo pi = probe[(size_t)q * max_lists + r];
        pos = write_list_blocks(wl, pos, r, list_gb0[cid], list_n[cid], pi, qcs, bsum, UNF);
    }
}

} // namespace rbq
