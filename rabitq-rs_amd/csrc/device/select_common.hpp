// select_common.hpp — the steps the three kernels that write the scan's input share: k_select and k_probes_given (select_given.hpp)
// and k_select_mfma (select_mfma.hpp).  Each step exists once, so that the probe constants, the stream entries and their bound agree
// bit for bit between the kernels by construction (tests/test_gpu_select_kernels_agree.py holds them together on one input):
//   radix_kth_key      the k-th smallest 64-bit (score, cid) key by eight passes of 8-bit histograms   (k_select, k_select_mfma's fallback)
//   bitonic_sort_keys  THE bitonic network over a power-of-two key window                              (k_select, sort_keys)
//   sort_keys          ascending sort of a window in LDS: rank sort when small, else the network         (k_select_mfma)
//   probe_info         per-probe constants of the IVF search, probe_info_given those of an MSTG list    (all three)
//   block_nvalid, stream_item   one entry of the block stream and its lower bound                       (all three)
//   write_list_blocks, serial_scan_excl256   one list's entries, serially, and where each thread's start (k_select, k_probes_given)
// k_select_mfma's tau search (a range-limited radix select over 32-bit approximate keys) and its four-entries-per-thread stream
// writer are other algorithms on the timed path and stay in select_mfma.hpp; the writer builds its entries with stream_item too.
#pragma once
#include "kernels.hpp"

namespace rbq {

// The key of rank *s_k (0-based, ascending) among key_of(i), i < n: eight passes from the top byte down, each a 256-bin histogram
// of the keys that match the prefix found so far.  hist: 256 words of LDS; *s_prefix = 0, *s_mask = 0 and *s_k are set (and a
// barrier passed) by the caller.  Every thread of the workgroup calls it and gets the same key.
template <class KeyOf>
__device__ __forceinline__ uint64_t radix_kth_key(KeyOf&& key_of, uint32_t n, uint32_t tid, uint32_t* hist, uint64_t* s_prefix, uint64_t* s_mask,
                                                  uint32_t* s_k) {
    for (int pass = 7; pass >= 0; --pass) {
        const int shift = pass * 8;
        hist[tid] = 0;
        __syncthreads();
        const uint64_t prefix = *s_prefix, mask = *s_mask;
        for (uint32_t i = tid; i < n; i += kThreads) {
            const uint64_t key = key_of(i);
            if ((key & mask) == prefix) atomicAdd(&hist[(uint32_t)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t k = *s_k, cum = 0, b = 0;
            for (; b < 256; ++b) {
                const uint32_t h = hist[b];
                if (k < cum + h) break;
                cum += h;
            }
            *s_k = k - cum;
            *s_prefix = prefix | ((uint64_t)b << shift);
            *s_mask = mask | (0xffull << shift);
        }
        __syncthreads();
    }
    return *s_prefix;
}

// Ascending bitonic sort of keys[0..cap2), cap2 a power of two (unused entries ~0).  fence_global: the window lives in global memory,
// where the workgroup's own writes of one stage are read back by other lanes in the next.
__device__ __forceinline__ void bitonic_sort_keys(uint64_t* keys, uint32_t cap2, uint32_t tid, bool fence_global) {
    for (uint32_t k = 2; k <= cap2; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < cap2; i += kThreads) {
                const uint32_t ixj = i ^ j;
                if (ixj > i) {
                    const uint64_t a = keys[i], b = keys[ixj];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { keys[i] = b; keys[ixj] = a; }
                }
            }
            if (fence_global) __threadfence_block();
            __syncthreads();
        }
}

// ascending sort of keys[0..n) in LDS (distinct keys; entries n..cap2-1 must be ~0 for the bitonic branch)
__device__ __forceinline__ void sort_keys(uint64_t* keys, uint32_t n, uint32_t cap2, uint32_t tid) {
    if (n <= 2 * kThreads) {
        // rank sort: the keys are distinct (they carry the list id), so the number of smaller keys IS the
        // position; every thread walks the n keys as LDS broadcasts — no barrier per compare-exchange stage
        uint64_t my[2] = {~0ull, ~0ull};
        uint32_t rk[2] = {0, 0};
#pragma unroll
        for (int u = 0; u < 2; ++u) if (tid + u * kThreads < n) my[u] = keys[tid + u * kThreads];
        const uint32_t wbase = tid & ~63u;
        // (unrolled: the loads of a group of keys are independent — one LDS round trip per 16 keys, not per key)
        if (n > (uint32_t)kThreads) {
#pragma unroll 8
            for (uint32_t j = 0; j < n; ++j) {
                const uint64_t kj = keys[j];
                rk[0] += kj < my[0] ? 1u : 0u;
                rk[1] += kj < my[1] ? 1u : 0u;
            }
        } else if (wbase < n) {
            const uint4* k2 = reinterpret_cast<const uint4*>(keys); // two keys per 16-byte read; slot n is ~0 (never smaller) when n is odd
            const uint32_t np2 = (n + 1) >> 1;
#pragma unroll 8
            for (uint32_t j = 0; j < np2; ++j) {
                const uint4 kk = k2[j];
                const uint64_t ka = ((uint64_t)kk.y << 32) | kk.x, kb = ((uint64_t)kk.w << 32) | kk.z;
                rk[0] += (ka < my[0] ? 1u : 0u) + (kb < my[0] ? 1u : 0u);
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 2; ++u) if (tid + u * kThreads < n) keys[rk[u]] = my[u];
        __syncthreads();
    } else {
        bitonic_sort_keys(keys, cap2, tid, false);
    }
}

// Per-probe constants of the IVF search (src/ivf.rs:1850-1857) from a list's canonical score — L2: the squared centroid distance; IP:
// the dot product, with the canonical squared centroid distance in dist_ip (not read for L2).
__device__ __forceinline__ ProbeInfo probe_info(int metric, float score, float dist_ip, uint32_t cid) {
    float dist, dot;
    // L2: score IS the centroid distance; the dot product only feeds the non-finite lower-bound
    // fallback of the IP metric (src/ivf.rs:2031-2042), so it is not computed here.
    if (metric == 0) { dist = score; dot = 0.0f; }
    else { dot = score; dist = dist_ip; }
    ProbeInfo pi;
    pi.g_add = metric == 0 ? dist : -dot;
    pi.g_err = sqrtf(dist);
    pi.dotqc = dot;
    pi.cid = cid;
    return pi;
}
// The same for a posting list the caller of an MSTG search names (search_posting_list_fastscan, src/mstg/index.rs:227-231): g_error = 0,
// and no dot product either.
__device__ __forceinline__ ProbeInfo probe_info_given(int metric, float score, uint32_t cid) {
    ProbeInfo pi;
    pi.g_add = metric == 0 ? score : -score;
    pi.g_err = 0.0f;
    pi.dotqc = 0.0f;
    pi.cid = cid;
    return pi;
}

// vectors of block b of a list of n: 32, but for the last block
__device__ __forceinline__ uint32_t block_nvalid(uint32_t n, uint32_t b) { return (b + 1 == ((n + 31u) >> 5)) ? n - b * 32u : 32u; }

// One entry of the block stream: block gblock of the probe of rank r with nvalid vectors, and the smallest lower bound any of them
// can have for this query (block_lbmin: what k_scan skips whole blocks by).  unfused: kVarPortable.
__device__ __forceinline__ StreamItem stream_item(uint32_t gblock, uint32_t r, uint32_t nvalid, const BlockSummary& bs, float g_add, float g_err,
                                                  const QueryConsts& qc, bool unfused) {
    StreamItem wi;
    wi.gblock = gblock;
    wi.rank_nvalid = (r << 6) | nvalid;
    wi.lbmin = block_lbmin(bs, g_add, g_err, qc, unfused);
    wi.pad = 0;
    return wi;
}

// the entries of the probe of rank r (n vectors from block gb on), one after the other from out[pos]; returns the position behind them
__device__ __forceinline__ uint64_t write_list_blocks(StreamItem* __restrict__ out, uint64_t pos, uint32_t r, uint32_t gb, uint32_t n,
                                                      const ProbeInfo& pi, const QueryConsts& qc, const BlockSummary* __restrict__ bsum,
                                                      bool unfused) {
    const uint32_t nb = (n + 31u) >> 5;
    for (uint32_t b = 0; b < nb; ++b) out[pos++] = stream_item(gb + b, r, block_nvalid(n, b), bsum[gb + b], pi.g_add, pi.g_err, qc, unfused);
    return pos;
}

// Exclusive prefix sum of one value per thread, serially by thread 0 through part[kThreads] in LDS (the writers it serves are not on
// a timed path); `total`, the sum of all values, is valid on thread 0 only.
__device__ __forceinline__ uint32_t serial_scan_excl256(uint32_t v, uint32_t* part, uint32_t tid, uint32_t& total) {
    part[tid] = v;
    __syncthreads();
    total = 0;
    if (tid == 0) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < kThreads; ++i) { const uint32_t x = part[i]; part[i] = run; run += x; }
        total = run;
    }
    __syncthreads();
    return part[tid];
}

} // namespace rbq
