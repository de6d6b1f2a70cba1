// k_mstg_range.hip — MSTG range search (include/ext/rbq_mstg_range.h, rbq_mstg_range_batch*): every vector of the selected
// posting lists whose binary estimate is below a radius, in scan order, and (distinct) one entry per id.  gfx950 only, wave64.
//
//   k_mstg_range<DT, UNF>   the scan.  k_range's tile walk (range.hpp: one workgroup of four scanning waves per query, half-wave hw of a
//     tile takes stream entry pos + hw of k_probes_given's block stream) under the MSTG candidate rule of k_scan's P.mstg branch
//     (src/mstg/index.rs:216-330): the estimate is the distance, a non-finite estimate drops the candidate, an L2 estimate below zero
//     becomes zero, and the distance is reported for both metrics.  No lower bound, no ex stage, no survivor compaction: a lane's
//     candidate is final when its lookups are, so a tile is
//       1. block bound: lbmin >= R (finite) -> nothing of the block is read.  With g_error = 0 the stream's lbmin (block_lbmin) is the
//          epilogue's own operation sequence on the extremes of every operand, f_error * 0 subtracted: a finite lbmin is <= the
//          estimate of every real vector of the block, so none of them is < R, clamped or not.  The skip that k_scan takes on MSTG
//          handles against its running threshold; here the threshold is the constant R.
//       2. factor rows + codes, the per-lane bound (the estimate is monotone in accu: est(amin), est(amax) finite and both >= R), LUT
//          lookups from LDS (scan_codes.hpp), the epilogue -> match;
//       3. one ballot per wave, the four counts through LDS (double-buffered by tile parity: ONE barrier per tile), and every match is
//          written at (matches so far + waves before + lanes before) while that is below the capacity; the count runs on.
//     The position is a function of the stream alone, never of wave timing: the same call gives the same rows every time.
//     DT: compile-time dimension (960 / 768 / 128; 0 = runtime).  UNF: the epilogue's first operation is not fused (kVarPortable); the
//     AVX2 and AVX-512 variants differ in the ex-code dot only, which this kernel never forms.
//     Dynamic LDS: lut[4 Dc] u8 at byte 0 | matches per wave [2][4] u32.
//
//   k_mstg_range_distinct   one workgroup per query over the row the scan wrote (total <= RBQ_MSTG_RANGE_DISTINCT_MAX):
//       A - C  rg_distinct_heads (range_common.hpp): keys, mr_sort by (id, estimate by value, rank), one flag in scan order per id —
//          the match the contract keeps is the smallest estimate, on equal values the earlier in scan order;
//       D  rg_walk_flags: the kept matches are copied from the scan's row to the caller's in rank order, up to the capacity.
//     A row whose total exceeds the limit is answered with UINT32_MAX and no entry: nothing is deduplicated on a prefix.
//     Dynamic LDS: id[np2] u64 | key[np2] u64 | flags[256] u32 | wave sums [4] u32, np2 = RBQ_MSTG_RANGE_DISTINCT_MAX: 65 KiB.
#include <hip/hip_runtime.h>

#include "rbq.h"
#include "ext/rbq_mstg_range.h"
#include "launch.hpp"
#include "kernels.hpp"
#include "range_common.hpp" // the steps shared with k_range and k_mstg_range_exact
#include "scan_codes.hpp"   // load_codes / lookup_codes / accumulate_block_rt

namespace rbq {

static_assert(RBQ_MSTG_RANGE_DISTINCT_MAX == kMstgRangeDistinctMax, "rbq_mstg_range.h and launch.hpp disagree");

template <int DT, bool UNF>
__global__ __launch_bounds__(kRangeThreads) void k_mstg_range(MstgRangeParams P) {
    extern __shared__ __align__(16) unsigned char smraw[];
    const uint32_t Dc = DT ? (uint32_t)DT : P.Dc;
    uint8_t* s_lut = smraw;
    uint32_t* s_wcnt = reinterpret_cast<uint32_t*>(smraw + (size_t)Dc * 4); // [2][4] matches per wave (buffer = tile & 1)
    // no static __shared__ in this kernel: the dynamic region must start at LDS address 0 (see lds_lut_ptr)
    const lds_lut_ptr lut0 = (lds_lut_ptr)(uint32_t)0; // == s_lut
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smraw != 0u) __builtin_trap();

    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t wave = tid >> 6, lane = tid & 63u, half = lane >> 5, l32 = lane & 31u, hw = tid >> 5;
    const size_t stride = (size_t)Dc * 4 + 384;
    const uint32_t cap = P.cap;
    const float R = P.R;
    {
        const uint4* src = reinterpret_cast<const uint4*>(P.lut + (size_t)q * Dc * 4);
        uint4* dst = reinterpret_cast<uint4*>(s_lut);
        for (uint32_t i = tid; i < Dc / 4; i += kRangeThreads) dst[i] = src[i];
    }
    const QueryConsts qc = P.consts[q];
    const ProbeInfo* probe = P.probe + (size_t)q * P.nprobe;
    const StreamItem* wl = P.wl + (size_t)q * P.wl_stride;
    const uint32_t ns = P.nstream[q];
    uint64_t* out_ids = P.out_ids + (size_t)q * cap;
    float* out_scores = P.out_scores + (size_t)q * cap;
    __syncthreads();

    // the estimate as it is: k_scan's lb_of without the error term, which g_error = 0 makes vanish
    auto est_of = [&](float f_add, float f_rescale, float g_add, float accu_f) -> float {
        float ip;
        return rg_estimate(qc, f_add, f_rescale, g_add, accu_f, UNF, ip);
    };
    const bool bound_ok = qc.amax <= 65535.0f && !P.no_block_bound; // (k_scan's condition: the accumulator cannot wrap)

    uint32_t total = 0, tile = 0; // uniform: matches so far
    for (uint32_t pos = 0; pos < ns; pos += (uint32_t)kRangeBlocks, ++tile) {
        const uint32_t buf = (tile & 1u) * 4u;
        StreamItem si;
        si.gblock = 0; si.rank_nvalid = 0; si.lbmin = 0.0f; si.pad = 0;
        bool live = pos + hw < ns; // (uniform in the half-wave, like everything derived from `si` alone)
        if (live) si = wl[pos + hw];
        const uint32_t nvalid = si.rank_nvalid & 63u;
        if (live && bound_ok && finite_f(si.lbmin) && si.lbmin >= R) live = false; // (a NaN radius skips nothing and matches nothing)
        const uint32_t slot = si.gblock * 32u + l32;
        bool match = false;
        float est = 0.0f;
        if (live) {
            const uint8_t* blk = P.blocks + (size_t)si.gblock * stride;
            CodeRegs<DT> cc;
            if (DT) load_codes<DT>(cc, blk, l32); // requested together with the factor rows
            const float* fac = reinterpret_cast<const float*>(blk + (size_t)Dc * 4);
            const float f_add = fac[l32], f_rescale = fac[32 + l32];
            const float g_add = probe[si.rank_nvalid >> 6].g_add;
            const bool valid = l32 < nvalid;
            bool prunable = !valid;
            if (bound_ok && valid) {
                const float a = est_of(f_add, f_rescale, g_add, qc.amin), b = est_of(f_add, f_rescale, g_add, qc.amax);
                prunable = finite_f(a) && finite_f(b) && fminf(a, b) >= R;
            }
            const uint32_t pm = (uint32_t)(__ballot(prunable) >> (half * 32u));
            if (pm != 0xffffffffu) { // uniform in the half-wave
                const uint32_t accu = (DT ? lookup_codes<DT>(cc, blk, l32, lut0) : accumulate_block_rt(blk, lut0, l32, Dc)) & 0xffffu;
                est = est_of(f_add, f_rescale, g_add, (float)accu);
                const bool fin = finite_f(est);               // `if distance.is_finite()`
                if (P.metric == 0) est = fmaxf(est, 0.0f);    // distance.max(0.0)
                match = valid && fin && est < R;
            }
        }
        // ---------------------------------------------------------------- matches, in (half-wave, lane) = stream order
        const unsigned long long bm = __ballot(match);
        if (lane == 0) s_wcnt[buf + wave] = (uint32_t)__popcll(bm);
        lds_barrier(); // the waves' counts of this tile (the other buffer is still being read by a wave behind)
        uint32_t wbase = 0, tm = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t c = s_wcnt[buf + j];
            wbase += (uint32_t)j < wave ? c : 0u;
            tm += c;
        }
        if (match) {
            const uint32_t at = total + wbase + (uint32_t)__popcll(bm & ((1ull << lane) - 1ull));
            if (at < cap) { // the count runs on past the capacity; writes at or beyond it are dropped
                out_ids[at] = P.ids[slot];
                out_scores[at] = est;
            }
        }
        total += tm;
    }
    for (uint32_t i = P.no_fill ? cap : (total < cap ? total : cap) + tid; i < cap; i += kRangeThreads) {
        out_ids[i] = ~0ull;
        out_scores[i] = __int_as_float(0x7fc00000);
    }
    if (tid == 0) P.out_counts[q] = total; // every match, also those beyond the capacity
}

__global__ __launch_bounds__(kThreads) void k_mstg_range_distinct(MstgRangeDistinctParams P) {
    extern __shared__ __align__(16) unsigned char smraw[];
    unsigned long long* k1 = reinterpret_cast<unsigned long long*>(smraw); // the id
    unsigned long long* k2 = k1 + kMstgRangeDistinctMax;                   // estimate key << 32 | scan rank
    uint32_t* s_keep = reinterpret_cast<uint32_t*>(k2 + kMstgRangeDistinctMax); // [kThreads] bit b of word t: rank 16 t + b is kept
    uint32_t* s_w = s_keep + kThreads;
    const uint32_t q = blockIdx.x, tid = threadIdx.x, cap = P.cap;
    const uint64_t* rids = P.raw_ids + (size_t)q * kMstgRangeDistinctMax;
    const float* rest = P.raw_scores + (size_t)q * kMstgRangeDistinctMax;
    uint64_t* out_ids = P.out_ids + (size_t)q * cap;
    float* out_scores = P.out_scores + (size_t)q * cap;
    const uint32_t total = P.raw_counts[q];
    uint32_t kept = 0;
    if (total != 0u && total <= kMstgRangeDistinctMax) { // (uniform)
        rg_distinct_heads(k1, k2, s_keep, rids, rest, total, tid); // ---- A to C
        // ---- D (r < total: only ranks of real entries were flagged)
        kept = rg_walk_flags(s_keep, s_w, tid, cap, [&](uint32_t at, uint32_t r) { out_ids[at] = rids[r]; out_scores[at] = rest[r]; });
    }
    rg_pad_row(out_ids, out_scores, kept < cap ? kept : cap, cap, tid, (uint32_t)kThreads);
    if (tid == 0) P.out_counts[q] = total > kMstgRangeDistinctMax ? 0xffffffffu : kept;
}

size_t mstg_range_lds_bytes(uint32_t Dc) { return (size_t)Dc * 4 + 8 * 4; }
size_t mstg_range_distinct_lds_bytes() { return (size_t)kMstgRangeDistinctMax * 16 + (size_t)kThreads * 4 + 16; }

namespace {
template <int DT, bool UNF>
hipError_t launch_mstg_range_i(const MstgRangeParams& P, int device, hipStream_t s) {
    static LdsAttrCache attr;
    const size_t lds = mstg_range_lds_bytes(P.Dc);
    hipError_t e = attr.ensure(reinterpret_cast<const void*>(&k_mstg_range<DT, UNF>), lds, device);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_mstg_range<DT, UNF>), dim3(P.nq), dim3(kRangeThreads), lds, s, P);
    return hipGetLastError();
}
} // namespace

hipError_t launch_mstg_range(const MstgRangeParams& P, int device, hipStream_t s) {
    if (P.nq == 0u || P.cap == 0u || P.Dc % 64u != 0u || mstg_range_lds_bytes(P.Dc) > kLdsPerWorkgroupMax) return hipErrorInvalidValue;
    if (P.numeric_variant == (uint32_t)kVarPortable) return launch_mstg_range_i<0, true>(P, device, s); // runtime dimension only
    if (P.numeric_variant != (uint32_t)kVarAvx512 && P.numeric_variant != (uint32_t)kVarAvx2) return hipErrorInvalidValue;
    if (P.D == P.Dc && P.D == 960) return launch_mstg_range_i<960, false>(P, device, s);
    if (P.D == P.Dc && P.D == 768) return launch_mstg_range_i<768, false>(P, device, s);
    if (P.D == P.Dc && P.D == 128) return launch_mstg_range_i<128, false>(P, device, s);
    return launch_mstg_range_i<0, false>(P, device, s);
}

hipError_t launch_mstg_range_distinct(const MstgRangeDistinctParams& P, int device, hipStream_t s) {
    static LdsAttrCache attr;
    if (P.nq == 0u || P.cap == 0u) return hipErrorInvalidValue;
    const size_t lds = mstg_range_distinct_lds_bytes();
    hipError_t e = attr.ensure(reinterpret_cast<const void*>(&k_mstg_range_distinct), lds, device);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mstg_range_distinct, dim3(P.nq), dim3(kThreads), lds, s, P);
    return hipGetLastError();
}

} // namespace rbq
