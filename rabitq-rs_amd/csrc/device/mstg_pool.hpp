// mstg_pool.hpp — what the kernels over an MSTG candidate pool share (gfx950): the refined search (k_mstg_refine.hip, DESIGN.md
// section 19) and the exact rerank of the pool (k_mstg_rerank.hip).  The pool is the binary scan's result over
// the identity slot map: entry r of a query is a global slot index (gblock * 32 + lane), ascending by estimate.  One copy of
//   mp_find_list  the list of an entry among the query's selected lists: its place j in the scan order and its g_add;
//   mp_rank       the rank of an entry: the contract's order among EQUAL estimates is (list order, vector order);
//   mr_sort       the bitonic network over two u64 arrays in LDS.
#pragma once
#include "kernels.hpp"

namespace rbq {

constexpr unsigned long long kMrDropped = ~0ull;
constexpr uint32_t kMpNoList = 0xffffffffu;

// The place j of `slot`'s list among the lc rows of the query's ProbeInfo (scan order), or kMpNoList: a slot out of range or a block
// of no selected list cannot come out of the scan, and such an entry is dropped.  *g_add: the float k_probes_given wrote for the list.
__device__ __forceinline__ uint32_t mp_find_list(const uint32_t* __restrict__ blk_list, const ProbeInfo* probe, uint32_t lc,
                                                 unsigned long long slot, uint64_t n_slots, float* g_add) {
    *g_add = 0.0f;
    if (slot >= n_slots) return kMpNoList;
    const uint32_t cid = blk_list[(uint32_t)(slot >> 5)];
    for (uint32_t j = 0; j < lc; ++j)
        if (probe[j].cid == cid) { *g_add = probe[j].g_add; return j; }
    return kMpNoList;
}

// The rank of pool entry r < cnt.  The scan returns the pool ascending by estimate (pest), but its heap leaves the order among EQUAL
// estimates to the sequence of its pushes and pops.  Equal estimates are neighbours, so the rank is the start of the entry's run of
// equal values plus the entries of the run with a smaller (j, slot).  j_of(i) / slot_of(i): the place of entry i's list and the low
// 32 bits of its slot.
template <class JOf, class SlotOf>
__device__ __forceinline__ uint32_t mp_rank(const float* pest, uint32_t cnt, uint32_t r, JOf j_of, SlotOf slot_of) {
    const float e = pest[r];
    const uint32_t j = j_of(r), sl = slot_of(r);
    uint32_t lo = r;
    while (lo > 0u && pest[lo - 1u] == e) --lo;
    uint32_t before = 0;
    for (uint32_t i = lo; i < cnt && pest[i] == e; ++i) {
        const uint32_t j2 = j_of(i), s2 = slot_of(i);
        if (i != r && (j2 < j || (j2 == j && s2 < sl))) ++before;
    }
    return lo + before;
}

// ascending bitonic sort of np2 (a power of two) entries by the workgroup: by (k1, k2), or by k2 alone with k1 carried along
template <bool BY_K1>
__device__ __forceinline__ void mr_sort(unsigned long long* k1, unsigned long long* k2, uint32_t np2, uint32_t tid) {
    for (uint32_t size = 2; size <= np2; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (uint32_t i = tid; i < (np2 >> 1); i += kThreads) {
                const uint32_t lo = ((i & ~(stride - 1u)) << 1) | (i & (stride - 1u)), hi = lo | stride;
                const bool up = (lo & size) == 0u;
                const unsigned long long a1 = k1[lo], b1 = k1[hi], a2 = k2[lo], b2 = k2[hi];
                const bool gt = BY_K1 ? (a1 > b1 || (a1 == b1 && a2 > b2)) : a2 > b2;
                if (gt == up) { k1[lo] = b1; k1[hi] = a1; k2[lo] = b2; k2[hi] = a2; }
            }
        }
    __syncthreads();
}

} // namespace rbq
