// range.hpp — k_range, the scan of the range search (gfx950, wave64): every vector of the probed lists whose distance is below a
// constant R, in scan order.
//
// Reference semantics: search_cluster_v2_batched (src/ivf.rs:2013-2127) with `distk` replaced by the constant R and no heap.  The
// loop then carries nothing from one candidate to the next: a candidate is skipped iff its lower bound is >= R, refined otherwise,
// and kept iff its (finite) distance is < R.  So there is no replay wave, no threshold to publish and no restart: all four waves
// scan, and the only order left to keep is the order of the OUTPUT (probe order, then position inside the list).
//
// One workgroup = one query.  Per tile, half-wave hw takes stream entry pos + hw (k_select_mfma's block stream, as k_scan reads it):
//   1. block bound: `lbmin >= R` (lbmin finite) -> the block's codes and factor rows are never read (k_scan's bound_ok conditions);
//   2. factor rows + codes, the per-lane bound lane_prunable, LUT lookups, k_scan's epilogue (lb_of) -> survivors `!(lb >= R)`;
//   3. the survivors' (slot, ip, g_add, est) are compacted in stream order through the half-waves' ballot masks;
//   4. 16-lane groups refine them (k_scan's refine_batch: the same ex-code dots and refined_distance, so the same bits);
//   5. every lane looks at the distance of ITS candidate: the matches of the tile are ranked by a prefix over the waves' match masks
//      and written at (matches so far + rank) while that is below the capacity; the count runs on.
// The append position is a function of the stream alone (tile, half-wave, lane), never of wave timing: the same call gives the same
// rows every time.
//
// The exact variant (XR = the element of the attached raw rows, kRawF32 / kRawF16 / kRawBf16; XIP = inner product; options
// range_exact / range_exact_radius_bits; instantiated in k_range_exact.hip): the matches of step 5 are only
// CANDIDATES.  Per tile that has one:
//   6. the candidates' ids are compacted in stream order (the prefix over the waves' match masks of step 5);
//   7. groups of eight lanes score one candidate each, 32 per round, exactly against its raw row: the chains of k_rerank_pool
//      (rerank_score.hpp) between the caller's unrotated query, held in LDS widened to f32, and the row; id >= n_raw scores NaN;
//   8. every candidate lane tests ITS exact score against X (distance < X, or dot > X for inner product; NaN never passes); a second
//      prefix over the waves' hit masks gives the write position (hits so far + rank), and the exact score is what is written.
// The total counts hits; SearchDiagnostics are those of steps 1 - 5 and depend on neither X nor the capacity.  A tile without a
// candidate costs nothing beyond step 5 (the test is uniform).  XR = kRangeEstimate compiles to the kernel without steps 6 - 8.
#pragma once
#include <type_traits>

#include "kernels.hpp"
#include "scan_codes.hpp"
#include "rerank_score.hpp"

namespace rbq {

// EX: compile-time ex_bits (0/2/6) when DT != 0; ignored (runtime P.ex_bits) when DT == 0.  V: numeric variant, instantiated for the
// runtime-dimension kernel only (as k_scan).
template <int DT, int EX, int V = kVarAvx512, int XR = kRangeEstimate, bool XIP = false>
__global__ __launch_bounds__(kRangeThreads) void k_range(std::conditional_t<XR == kRangeEstimate, RangeParams, RangeExactParams> P) {
    constexpr bool kExact = XR != kRangeEstimate;
    extern __shared__ __align__(16) unsigned char smraw[];
    const uint32_t Dc = DT ? (uint32_t)DT : P.Dc; // code/LUT dimension (x64)
    const uint32_t D = DT ? (uint32_t)DT : P.D;   // padded_dim (ex codes, rotated query)
    const uint32_t ex_bits = DT ? (uint32_t)EX : P.ex_bits;
    const uint32_t nunits = ex_w4(D, ex_bits), qlen = ex_qlen(D, ex_bits);
    uint8_t* s_lut = smraw;
    float* s_q = reinterpret_cast<float*>(smraw + (size_t)Dc * 4);
    uint32_t* c_slot = reinterpret_cast<uint32_t*>(s_q + qlen); // [kRangeCand] the tile's survivors, stream order
    float* c_ip = reinterpret_cast<float*>(c_slot + kRangeCand);
    float* c_gadd = c_ip + kRangeCand;
    float* c_d = c_gadd + kRangeCand;
    uint32_t* s_mask = reinterpret_cast<uint32_t*>(c_d + kRangeCand); // [2][kRangeBlocks] survivor masks (buffer = tile & 1)
    uint32_t* s_wcnt = s_mask + 2 * kRangeBlocks;                     // [4] matches per wave | [4] finite distances per wave
    uint32_t* s_nskip = s_wcnt + 8;
    // the exact variant's region (types.hpp: range_exact_lds_bytes), 16-byte aligned; never touched when !kExact
    unsigned long long* x_id = reinterpret_cast<unsigned long long*>(s_nskip + 4); // [kRangeCand] the tile's candidates, stream order
    float* x_sc = reinterpret_cast<float*>(x_id + kRangeCand);                     // [kRangeCand] their exact scores
    uint32_t* s_hcnt = reinterpret_cast<uint32_t*>(x_sc + kRangeCand);             // [4] hits per wave
    float* x_q = reinterpret_cast<float*>(s_hcnt + 4);                             // [dim] the caller's query, widened
    // no static __shared__ in this kernel: the dynamic region must start at LDS address 0 (see lds_lut_ptr)
    const lds_lut_ptr lut0 = (lds_lut_ptr)(uint32_t)0; // == s_lut
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smraw != 0u) __builtin_trap();

    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t wave = tid >> 6, lane = tid & 63u, half = lane >> 5, l32 = lane & 31u, hw = tid >> 5;
    const size_t stride = (size_t)Dc * 4 + 384;
    const size_t exb = ex_bytes_dev(D, ex_bits);
    const uint32_t cap = P.top_k;
    const float R = P.R;
    {
        const uint4* src = reinterpret_cast<const uint4*>(P.lut + (size_t)q * Dc * 4);
        uint4* dst = reinterpret_cast<uint4*>(s_lut);
        for (uint32_t i = tid; i < Dc / 4; i += kRangeThreads) dst[i] = src[i];
        // the rotated query, zero-padded to ex_qlen: every code slot of every unit has a (zero) partner
        const float4* rs = reinterpret_cast<const float4*>(P.rot + (size_t)q * D); // (D % 4 == 0: padded_dim is a multiple of 64)
        float4* rd = reinterpret_cast<float4*>(s_q);
        for (uint32_t i = tid; i < qlen / 4; i += kRangeThreads) rd[i] = i < D / 4 ? rs[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (tid == 0) *s_nskip = 0;
        if constexpr (kExact) copy_query_widened<kRangeThreads>(x_q, P.queries, P.query_dtype, (size_t)q * P.dim, P.dim, tid);
    }
    const QueryConsts qc = P.consts[q];
    const ProbeInfo* probe = P.probe + (size_t)q * P.nprobe;
    const StreamItem* wl = P.wl + (size_t)q * P.wl_stride;
    const uint32_t ns = P.nstream[q];
    __syncthreads();

    struct Meta { float f_add, f_rescale, f_error, g_add, g_err, dotqc; };
    // the epilogue's exact operation sequence (k_scan's lb_of: compute_batch_distances_u16, first op fused or not per variant)
    auto lb_of = [&](const Meta& m, float accu_f, float& ip, float& est) -> float {
        ip = epi_ip(qc.delta, accu_f, qc.sum_vl, V == kVarPortable);
        const float tt = ip + qc.k1x;
        const float rs = m.f_rescale * tt;
        est = m.f_add + m.g_add;
        est = est + rs;
        const float er = m.f_error * m.g_err;
        return est - er;
    };
    // k_scan's conditions: the accumulator cannot wrap, and filtered diagnostics need every candidate's filter test
    const bool bound_ok = qc.amax <= 65535.0f && !(P.filter && P.diag) && !P.no_block_bound;
    const bool count_skips = P.diag != nullptr;

    uint32_t n_skip = 0;                       // per thread
    uint32_t n_ext = 0, n_est = 0, total = 0;  // uniform: survivors, finite distances, matches so far
    uint32_t tile = 0;
    for (uint32_t pos = 0; pos < ns; pos += (uint32_t)kRangeBlocks, ++tile) {
        const uint32_t buf = (tile & 1u) * (uint32_t)kRangeBlocks;
        // ---------------------------------------------------------------- scan: one stream entry per half-wave
        StreamItem si;
        si.gblock = 0; si.rank_nvalid = 0; si.lbmin = 0.0f; si.pad = 0;
        bool live = pos + hw < ns; // (uniform in the half-wave, like everything derived from `si` alone)
        if (live) si = wl[pos + hw];
        const uint32_t nvalid = si.rank_nvalid & 63u;
        // block_lbmin(): finite means every real vector of the block has a finite lower bound >= lbmin; -inf means "never skip"
        if (live && bound_ok && finite_f(si.lbmin) && si.lbmin >= R) {
            live = false;
            if (count_skips && l32 == 0) n_skip += nvalid;
        }
        const uint32_t slot = si.gblock * 32u + l32;
        bool surv = false;
        float ip = 0.0f, est = 0.0f, g_add = 0.0f;
        if (live) {
            const uint8_t* blk = P.blocks + (size_t)si.gblock * stride;
            CodeRegs<DT> cc;
            if (DT) load_codes<DT>(cc, blk, l32); // requested together with the factor rows
            const float* fac = reinterpret_cast<const float*>(blk + (size_t)Dc * 4);
            const ProbeInfo pi = probe[si.rank_nvalid >> 6];
            Meta m;
            m.f_add = fac[l32]; m.f_rescale = fac[32 + l32]; m.f_error = fac[64 + l32];
            m.g_add = pi.g_add; m.g_err = pi.g_err; m.dotqc = pi.dotqc;
            g_add = m.g_add;
            bool valid = l32 < nvalid;
            if (valid && P.filter) {
                const uint32_t id32 = (uint32_t)P.ids[slot];
                valid = ((uint64_t)id32 < P.filter_nbits) && ((P.filter[id32 >> 5] >> (id32 & 31u)) & 1u);
            }
            // per-lane bound (k_scan's lane_prunable): lb is monotone in accu, so min(lb(amin), lb(amax)) <= lb(true accu); when that
            // reaches R for every lane of the block, nothing is looked up
            bool prunable = l32 >= nvalid;
            if (bound_ok && !prunable) {
                float d0, d1;
                const float a = lb_of(m, qc.amin, d0, d1), b = lb_of(m, qc.amax, d0, d1);
                prunable = finite_f(a) && finite_f(b) && fminf(a, b) >= R;
            }
            const uint32_t pm = (uint32_t)(__ballot(prunable) >> (half * 32u));
            if (!bound_ok || pm != 0xffffffffu) { // uniform in the half-wave
                const uint32_t accu = (DT ? lookup_codes<DT>(cc, blk, l32, lut0) : accumulate_block_rt(blk, lut0, l32, Dc)) & 0xffffu;
                float lb = lb_of(m, (float)accu, ip, est);
                // the reference's replacement of a non-finite bound (src/ivf.rs:2031-2042); what it gives may be NaN again, and a NaN
                // bound is never `>= R`
                if (!finite_f(lb)) lb = P.metric == 0 ? 0.0f : -(m.dotqc + qc.qnorm);
                surv = valid && !(lb >= R);
            }
            if (valid && !surv) ++n_skip;
        }
        const uint32_t mask32 = (uint32_t)(__ballot(surv) >> (half * 32u));
        if (l32 == 0) s_mask[buf + hw] = mask32;
        lds_barrier(); // A: the tile's survivor masks
        uint32_t S = 0, base = 0;
#pragma unroll
        for (int j = 0; j < kRangeBlocks; ++j) {
            const uint32_t c = __popc(s_mask[buf + j]);
            base += (uint32_t)j < hw ? c : 0u;
            S += c;
        }
        if (S == 0) continue; // (uniform: the masks are the same for every thread)
        float d = est; // ex_bits == 0: the estimate is the distance
        if (ex_bits) {
            // ------------------------------------------------------------ compaction in stream order, refine by 16-lane groups
            const uint32_t cp = base + __popc(mask32 & ((1u << l32) - 1u));
            if (surv) { c_slot[cp] = slot; c_ip[cp] = ip; c_gadd[cp] = g_add; }
            lds_barrier(); // B: the survivors' operands
            const uint32_t gl = tid & 15u;
            for (uint32_t p = tid >> 4; p < S; p += (uint32_t)(kRangeThreads / 16)) {
                const uint32_t sl = c_slot[p];
                const uint8_t* ex = P.ex_codes + (size_t)sl * exb;
                float sacc, fa, fr;
                if constexpr (V != kVarAvx512) {
                    fa = P.f_add_ex[sl]; fr = P.f_rescale_ex[sl];
                    sacc = ex_dot_var_rt<V>(ex, s_q, gl, nunits, D / 16, ex_bits); // (already the group's sum)
                } else if (nunits <= (uint32_t)kExRegUnits) {
                    uint4 u[kExRegUnits];
                    ex_load_all(u, ex, gl, nunits);
                    fa = P.f_add_ex[sl]; fr = P.f_rescale_ex[sl];
                    sacc = ex_bits == 6 ? ex_dot_all<6>(u, s_q, gl, nunits) : ex_dot_all<2>(u, s_q, gl, nunits);
                } else {
                    fa = P.f_add_ex[sl]; fr = P.f_rescale_ex[sl];
                    sacc = ex_bits == 6 ? ex_dot_units<6>(ex, s_q, gl, nunits) : ex_dot_units<2>(ex, s_q, gl, nunits);
                }
                if constexpr (V == kVarAvx512) sacc = group16_reduce(sacc);
                if (gl == 0) c_d[p] = refined_distance(qc.scale, c_ip[p], sacc, qc.kbx, fa, c_gadd[p], fr);
            }
            lds_barrier(); // C: the refined distances
            if (surv) d = c_d[cp];
        }
        // ---------------------------------------------------------------- matches, in (half-wave, lane) = stream order
        const bool fin = surv && finite_f(d);
        const bool match = fin && d < R;
        const unsigned long long bm = __ballot(match), bf = __ballot(fin);
        if (lane == 0) { s_wcnt[wave] = (uint32_t)__popcll(bm); s_wcnt[4 + wave] = (uint32_t)__popcll(bf); }
        lds_barrier(); // D: the waves' counts
        uint32_t wbase = 0, tm = 0, tf = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t c = s_wcnt[j];
            wbase += (uint32_t)j < wave ? c : 0u;
            tm += c;
            tf += s_wcnt[4 + j];
        }
        if constexpr (!kExact) {
            if (match) {
                const uint32_t at = total + wbase + (uint32_t)__popcll(bm & ((1ull << lane) - 1ull));
                if (at < cap) { // the count runs on past the capacity; writes at or beyond it are dropped
                    P.out_ids[(size_t)q * cap + at] = P.ids[slot];
                    P.out_scores[(size_t)q * cap + at] = P.metric == 0 ? d : -d;
                }
            }
            n_ext += S; n_est += tf; total += tm;
        } else {
            n_ext += S; n_est += tf;
            if (tm == 0) continue; // (uniform) no candidate in this tile
            // ------------------------------------------------------------ the candidates' ids, compacted in stream order
            const uint32_t mp = wbase + (uint32_t)__popcll(bm & ((1ull << lane) - 1ull)); // < tm <= kRangeCand
            unsigned long long id = 0;
            if (match) { id = P.ids[slot]; x_id[mp] = id; }
            lds_barrier(); // E: the candidates' ids
            // ------------------------------------------------------------ exact scores: eight lanes per candidate, 32 per round
            {
                const uint32_t j = lane & 7u, gbase = lane & ~7u;
                for (uint32_t c0 = 0; c0 < tm; c0 += (uint32_t)(kRangeThreads / 8)) { // (uniform trip count: every lane scores)
                    const uint32_t c = c0 + (tid >> 3);
                    const bool have = c < tm;
                    const unsigned long long cid = have ? x_id[c] : ~0ull;
                    const bool act = have && cid < P.n_raw;
                    const float sum = rp_score_row<XIP, kExact ? XR : kRawF32>(P.raw, cid, act, x_q, P.dim, j, gbase, P.raw_by_element != 0u);
                    if (have && j == 0u) x_sc[c] = act ? sum : __int_as_float(0x7fc00000);
                }
            }
            lds_barrier(); // F: the exact scores
            float xs = 0.0f;
            bool hit = false;
            if (match) {
                xs = x_sc[mp];
                hit = XIP ? xs > P.X : xs < P.X; // (a NaN score, and any score against a NaN X, never passes)
            }
            const unsigned long long bh = __ballot(hit);
            if (lane == 0) s_hcnt[wave] = (uint32_t)__popcll(bh);
            lds_barrier(); // G: the waves' hit counts
            uint32_t hbase = 0, th = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t c = s_hcnt[w];
                hbase += (uint32_t)w < wave ? c : 0u;
                th += c;
            }
            if (hit) {
                const uint32_t at = total + hbase + (uint32_t)__popcll(bh & ((1ull << lane) - 1ull));
                if (at < cap) { // the count runs on past the capacity; writes at or beyond it are dropped
                    P.out_ids[(size_t)q * cap + at] = id;
                    P.out_scores[(size_t)q * cap + at] = xs;
                }
            }
            total += th;
        }
    }
    if (P.diag && n_skip) atomicAdd(s_nskip, n_skip);
    __syncthreads();
    for (uint32_t i = (total < cap ? total : cap) + tid; i < cap; i += kRangeThreads) {
        P.out_ids[(size_t)q * cap + i] = ~0ull;
        P.out_scores[(size_t)q * cap + i] = __int_as_float(0x7fc00000);
    }
    if (tid == 0) {
        P.out_counts[q] = total; // every match, also those beyond the capacity
        if (P.diag) {
            P.diag[(size_t)q * 3 + 0] = n_est;
            P.diag[(size_t)q * 3 + 1] = *s_nskip;
            P.diag[(size_t)q * 3 + 2] = ex_bits ? n_ext : 0;
        }
    }
}

} // namespace rbq
