// canon_score.hpp — query x centroid scores in the reference's canonical order (math::l2_distance_sqr / dot in their AVX2 lane order,
// src/math.rs:154-245: eight strided accumulators, unfused multiply and add, the accumulators summed 0..7 from -0.0, a scalar tail),
// for single pairs and for the entries of a shortlist.  Used by the probe selection (select_mfma.hpp, select_given.hpp) and the MSTG
// search.  k_rank_scores (query_kernels.hpp) keeps the same order in registers: its accumulators are an array per thread, not lanes.
#pragma once
#include "kernels.hpp"

namespace rbq {

#ifndef RBQ_CANON_UNROLL
#define RBQ_CANON_UNROLL 4 // 16-byte loads a lane keeps in flight in the canonical rescoring pass
#endif

// Canonical-order score of one (query, list) pair on 2 lanes: lane h owns the reference's accumulators
// 4h..4h+3 (elements 8t+4h..8t+4h+3, one 16-byte load per step); the final sum adds the eight accumulators
// in order 0..7 starting from -0.0 (Rust iter().sum()), then the scalar tail.  D % 4 == 0.
template <int METRIC>
__device__ __forceinline__ float canon_pair2(const float* qrot, const float* __restrict__ c, uint32_t D, uint32_t h) {
    const uint32_t Dmain = D & ~7u;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll RBQ_CANON_UNROLL
    for (uint32_t i = 4 * h; i < Dmain; i += 8) {
        const float4 cv = *reinterpret_cast<const float4*>(c + i);
        const float4 qv = *reinterpret_cast<const float4*>(qrot + i);
        float p0, p1, p2, p3;
        if (METRIC == 0) {
            const float d0 = qv.x - cv.x, d1 = qv.y - cv.y, d2 = qv.z - cv.z, d3 = qv.w - cv.w;
            p0 = d0 * d0; p1 = d1 * d1; p2 = d2 * d2; p3 = d3 * d3;
        } else {
            p0 = qv.x * cv.x; p1 = qv.y * cv.y; p2 = qv.z * cv.z; p3 = qv.w * cv.w;
        }
        a0 = a0 + p0; a1 = a1 + p1; a2 = a2 + p2; a3 = a3 + p3;
    }
    float sum = 0.0f;
    if (Dmain) {
        sum = -0.0f;
        sum = sum + __shfl(a0, 0, 2); sum = sum + __shfl(a1, 0, 2); sum = sum + __shfl(a2, 0, 2); sum = sum + __shfl(a3, 0, 2);
        sum = sum + __shfl(a0, 1, 2); sum = sum + __shfl(a1, 1, 2); sum = sum + __shfl(a2, 1, 2); sum = sum + __shfl(a3, 1, 2);
    }
    for (uint32_t i = Dmain; i < D; ++i) {
        float p;
        if (METRIC == 0) {
            const float d = qrot[i] - c[i];
            p = d * d;
        } else {
            p = qrot[i] * c[i];
        }
        sum = sum + p;
    }
    return sum;
}

// Inner-product metric: the canonical dot (the score) and the canonical squared distance (g_error needs it for
// every probed list) of one (query, list) pair in ONE pass over the centroid row; same accumulators, same order
// as canon_pair2<1> and canon_pair2<0>.
__device__ __forceinline__ void canon_pair2_ip_l2(const float* qrot, const float* __restrict__ c, uint32_t D, uint32_t h,
                                                  float& dot, float& l2) {
    const uint32_t Dmain = D & ~7u;
    float a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
#pragma unroll 4
    for (uint32_t i = 4 * h; i < Dmain; i += 8) {
        const float4 cv = *reinterpret_cast<const float4*>(c + i);
        const float4 qv = *reinterpret_cast<const float4*>(qrot + i);
        const float q4[4] = {qv.x, qv.y, qv.z, qv.w}, c4[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float p = q4[k] * c4[k];
            const float d = q4[k] - c4[k];
            const float r = d * d;
            a[k] = a[k] + p;
            b[k] = b[k] + r;
        }
    }
    float s0 = 0.0f, s1 = 0.0f;
    if (Dmain) {
        s0 = -0.0f; s1 = -0.0f;
#pragma unroll
        for (int l = 0; l < 2; ++l)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                s0 = s0 + __shfl(a[k], l, 2);
                s1 = s1 + __shfl(b[k], l, 2);
            }
    }
    for (uint32_t i = Dmain; i < D; ++i) {
        const float p = qrot[i] * c[i];
        const float d = qrot[i] - c[i];
        const float r = d * d;
        s0 = s0 + p;
        s1 = s1 + r;
    }
    dot = s0; l2 = s1;
}

// The end of a canonical sum whose eight accumulators sit on the 8 lanes of a group (lane a: elements a, a + 8, ... below Dmain; acc
// the score's, acc2 the squared distance's of an inner-product list): from -0.0 the accumulators are added in order 0..7, then the
// scalar tail Dmain..D.  metric 0: sum is the squared distance; metric 1: sum is the dot product and sum2 the squared distance.
__device__ __forceinline__ void canon_finish8(float acc, float acc2, const float* qrot, const float* c, uint32_t D, uint32_t Dmain, int metric,
                                              float& sum_out, float& sum2_out) {
    float sum = 0.0f, sum2 = 0.0f; // (locals, stored once at the end: sums kept behind the references end up in scratch memory)
    if (Dmain) {
        sum = -0.0f; sum2 = -0.0f;
#pragma unroll
        for (int l = 0; l < 8; ++l) {
            sum = sum + __shfl(acc, l, 8);
            sum2 = sum2 + __shfl(acc2, l, 8);
        }
    }
    for (uint32_t i = Dmain; i < D; ++i) { // scalar tail
        const float qv = qrot[i], cv = c[i];
        const float d = qv - cv;
        const float r2 = d * d;
        if (metric == 0) sum = sum + r2;
        else {
            const float p = qv * cv;
            sum = sum + p;
            sum2 = sum2 + r2;
        }
    }
    sum_out = sum; sum2_out = sum2;
}

// ---- canonical scores of shortlist entries ----------------------------------------------------------------------------
// Both scorers overwrite keys[e] (approximate key | cid) with the EXACT (score, cid) key of entry e = idx_of(j), j < m, and
// park the canonical squared distance of an inner-product list in the (no longer needed) approximate row.  Same
// accumulators, same order, bit-identical results.
//   pairs : 2 lanes per list straight from global memory, 128 lists per round — every lane walks its row in dependent
//           batches of 16-byte loads, each of which uses a quarter of the 32 cache lines it touches: the round-2 scorer, right
//           when MANY lists are scored (it is bound by the L1 fill rate of those quarter-used lines)
//   staged: `rows` lists at a time are loaded by the whole workgroup with fully coalesced 16-byte loads into LDS (one
//           round trip, whole lines), then 8 lanes per list — one per accumulator of src/math.rs:216-245 — run the 120-step
//           add chains from LDS: ~5 us for a handful of lists against ~45 us for a pair round.  What the lazy selection uses.
template <typename IdxFn>
__device__ __forceinline__ void canon_score_pairs(uint64_t* keys, const float* qrot, const float* __restrict__ cent, uint32_t D, int metric,
                                                  float* grow, uint32_t m, uint32_t tid, IdxFn idx_of) {
    const uint32_t l2 = tid & 1u, grp = tid >> 1;
    for (uint32_t i0 = 0; i0 < m; i0 += kThreads / 2) {
        const uint32_t j = i0 + grp;
        uint32_t cid = 0, e = 0;
        float s = 0.0f;
        if (j < m) {
            e = idx_of(j);
            cid = (uint32_t)keys[e];
            const float* c = cent + (size_t)cid * D;
            if (metric == 0) s = canon_pair2<0>(qrot, c, D, l2);
            else {
                float dl2;
                canon_pair2_ip_l2(qrot, c, D, l2, s, dl2);
                if (l2 == 0) grow[cid] = dl2;
            }
        }
        if (j < m && l2 == 0) keys[e] = make_key(s, cid, metric);
    }
}
template <typename IdxFn>
__device__ __forceinline__ void canon_score_staged(uint64_t* keys, const float* qrot, const float* __restrict__ cent, uint32_t D, int metric,
                                                   float* grow, uint32_t m, uint32_t tid, float* rows, uint32_t RB, IdxFn idx_of) {
    const uint32_t Dp = D + 8u, Dmain = D & ~7u, nv4 = D >> 2; // (+8 floats: the 8 lanes of consecutive rows hit distinct banks)
    for (uint32_t base = 0; base < m; base += RB) {
        const uint32_t nr = m - base < RB ? m - base : RB;
        // (four 16-byte loads per thread in flight: as a plain copy loop every iteration waited for its load in front of its ds_write)
        for (uint32_t x0 = tid; x0 < nr * nv4; x0 += 4 * kThreads) {
            float4 t4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t x = x0 + (uint32_t)u * kThreads;
                t4[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (x < nr * nv4) {
                    const uint32_t r = x / nv4, j4 = x - r * nv4;
                    const uint32_t cid = (uint32_t)keys[idx_of(base + r)];
                    t4[u] = *reinterpret_cast<const float4*>(cent + (size_t)cid * D + 4 * j4);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t x = x0 + (uint32_t)u * kThreads;
                if (x < nr * nv4) {
                    const uint32_t r = x / nv4, j4 = x - r * nv4;
                    *reinterpret_cast<float4*>(rows + (size_t)r * Dp + 4 * j4) = t4[u];
                }
            }
        }
        __syncthreads();
        if (tid < nr * 8u) {
            const uint32_t r = tid >> 3, a = tid & 7u;
            const float* c = rows + (size_t)r * Dp;
            float acc = 0.0f, acc2 = 0.0f;
            if (metric == 0) {
#pragma unroll 8
                for (uint32_t i = a; i < Dmain; i += 8) {
                    const float d = qrot[i] - c[i];
                    const float p = d * d;
                    acc = acc + p;
                }
            } else {
#pragma unroll 8
                for (uint32_t i = a; i < Dmain; i += 8) {
                    const float qv = qrot[i], cv = c[i];
                    const float p = qv * cv;
                    const float d = qv - cv;
                    const float r2 = d * d;
                    acc = acc + p;
                    acc2 = acc2 + r2;
                }
            }
            float sum, sum2;
            canon_finish8(acc, acc2, qrot, c, D, Dmain, metric, sum, sum2);
            if (a == 0) {
                const uint32_t e = idx_of(base + r);
                const uint32_t cid = (uint32_t)keys[e];
                keys[e] = make_key(sum, cid, metric);
                if (metric == 1) { grow[cid] = sum2; __threadfence_block(); }
            }
        }
        __syncthreads();
    }
}

//   octets: 8 lanes per list straight from global memory, one per accumulator (4-byte loads, the 8 lanes of a list read 32
//           contiguous bytes per step), 32 lists per round, 30 loads in flight per lane: a third of a pair round's time for
//           up to 32 lists — the middle ground between `staged` (<= 8 lists) and `pairs` (> 64).
template <typename IdxFn>
__device__ __forceinline__ void canon_score_octets(uint64_t* keys, const float* qrot, const float* __restrict__ cent, uint32_t D, int metric,
                                                   float* grow, uint32_t m, uint32_t tid, IdxFn idx_of) {
    const uint32_t a = tid & 7u, grp = tid >> 3, Dmain = D & ~7u;
    for (uint32_t i0 = 0; i0 < m; i0 += kThreads / 8) {
        const uint32_t j = i0 + grp;
        if (j < m) { // uniform per 8-lane group
            const uint32_t e = idx_of(j);
            const uint32_t cid = (uint32_t)keys[e];
            const float* c = cent + (size_t)cid * D;
            float acc = 0.0f, acc2 = 0.0f;
            // explicit two-phase steps (all loads of a batch, then its adds in order): left to itself hipcc waits for every
            // load in front of its add
            constexpr int KB = 24;
            for (uint32_t base = a; base < Dmain; base += 8 * KB) {
                float cv[KB];
#pragma unroll
                for (int k = 0; k < KB; ++k) cv[k] = base + 8u * k < Dmain ? c[base + 8u * k] : 0.0f;
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    if (base + 8u * k < Dmain) {
                        const float qv = qrot[base + 8u * k];
                        if (metric == 0) {
                            const float d = qv - cv[k];
                            const float p = d * d;
                            acc = acc + p;
                        } else {
                            const float p = qv * cv[k];
                            const float d = qv - cv[k];
                            const float r2 = d * d;
                            acc = acc + p;
                            acc2 = acc2 + r2;
                        }
                    }
                }
            }
            float sum, sum2;
            canon_finish8(acc, acc2, qrot, c, D, Dmain, metric, sum, sum2);
            if (a == 0) {
                keys[e] = make_key(sum, cid, metric);
                if (metric == 1) grow[cid] = sum2;
            }
        }
    }
}

// wave-wide minimum of one u32 per lane, on DPP (row_shr 1/2/4/8, row_bcast 15/31; the result is read from lane 63)
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x) {
    const int id = -1; // 0xffffffff: identity of the unsigned minimum
    uint32_t t;
    t = (uint32_t)__builtin_amdgcn_update_dpp(id, (int)x, 0x111, 0xf, 0xf, false); x = t < x ? t : x;
    t = (uint32_t)__builtin_amdgcn_update_dpp(id, (int)x, 0x112, 0xf, 0xf, false); x = t < x ? t : x;
    t = (uint32_t)__builtin_amdgcn_update_dpp(id, (int)x, 0x114, 0xf, 0xf, false); x = t < x ? t : x;
    t = (uint32_t)__builtin_amdgcn_update_dpp(id, (int)x, 0x118, 0xf, 0xf, false); x = t < x ? t : x;
    t = (uint32_t)__builtin_amdgcn_update_dpp(id, (int)x, 0x142, 0xa, 0xf, false); x = t < x ? t : x;
    t = (uint32_t)__builtin_amdgcn_update_dpp(id, (int)x, 0x143, 0xc, 0xf, false); x = t < x ? t : x;
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

} // namespace rbq
