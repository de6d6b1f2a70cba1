// bf.hpp — kernels of the brute-force index (rbq_bf_search_batch): BruteForceRabitqIndex::search_internal
// (reference src/brute_force.rs:545-650).  Two kernels per (sub-batch of queries, chunk of vectors):
//
//   k_bf_dist    every (query, vector) distance of the chunk, in the reference's arithmetic, into a [nq][nv] f32 workspace.
//                Filtered-out vectors get NaN: the reference `continue`s on both, so a filtered vector and a non-finite
//                distance are the same thing to the heap below.
//   k_bf_select  one wave per query: the reference's BinaryHeap push / pop loop over the query's distances in id order
//                (LdsHeap of topk.hpp: Rust's std BinaryHeap operation for operation), then into_sorted_vec.
//
// Arithmetic (brute_force.rs:581-615; the crate is plain scalar Rust without fast-math, so no build of it reorders or fuses):
//   bd   = sum_i (float)bit_i * rq_i        sequential from +0.0f, multiply then add (never fused)
//   ed   = sum_i (float)code_i * rq_i       the same
//   ex == 0:  dist = (f_add + 0.0f) + f_rescale * (bd + k1x)
//   ex >  0:  dist = (f_add_ex + 0.0f) + f_rescale_ex * (((bs * bd) + ed) + kbx)
// k1x, kbx, bs = QueryPrecomputed (brute_force.rs:79-96): the IVF path's constants, computed by k_prep (QueryConsts).
// The translation unit is compiled with -ffp-contract=off; tests/test_bruteforce_host.py checks that the compiled kernels
// contain no v_fma / v_fmac / v_pk_fma / v_dot instruction and no scratch.
//
// Tiling of k_bf_dist: a workgroup owns kBfVec vectors (lane = vector) x kBfQ queries.  The rotated queries of the tile are
// staged in LDS dimension-major ([dim][query]), kBfChunk dimensions at a time, so that one dimension of all kBfQ queries is a
// few broadcast ds_read_b128.  Each lane unpacks its sign bits and ex codes for 16 dimensions once (6-bit: 12 bytes, 2-bit:
// 4 bytes, §A5 layouts) and then runs the 2 x kBfQ running sums of the tile, two queries per v_pk_mul_f32 / v_pk_add_f32:
// packing keeps IEEE rounding per half; only contraction would change the result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "topk.hpp"
#include "types.hpp"

namespace rbq {

constexpr uint32_t kBfVec = 256;   // vectors per workgroup of k_bf_dist (one per lane)
constexpr uint32_t kBfQ = 32;      // queries per workgroup of k_bf_dist
constexpr uint32_t kBfChunk = 64;  // dimensions of the query tile staged in LDS at a time

typedef float bf_f2 __attribute__((ext_vector_type(2)));

// code of dimension j (0..15) of a 16-dimension unit, §A5 layouts (rbq_build.cpp pack_ex2 / pack_ex6)
template <int EX>
__device__ __forceinline__ float bf_ex_code(uint32_t lo0, uint32_t lo1, uint32_t hi, int j) {
    const uint32_t g = (uint32_t)j >> 2, i = (uint32_t)j & 3u;
    const uint32_t top = (hi >> (8u * i + 2u * g)) & 3u;
    if (EX == 2) return (float)top;
    // low nibbles: byte b of the 8-byte word holds dimension b (bits 0-3) and dimension b + 8 (bits 4-7)
    const uint32_t b = (uint32_t)j & 7u, sh = j < 8 ? 0u : 4u;
    const uint32_t lo = ((b < 4 ? lo0 >> (8u * b) : lo1 >> (8u * (b - 4u))) >> sh) & 15u;
    return (float)(lo | (top << 4));
}

// one 16-dimension unit of one vector against the kBfQ queries of the tile: sq = LDS tile [kBfChunk][kBfQ], d0 = first
// dimension of the unit inside the staged chunk
template <int EX>
__device__ __forceinline__ void bf_unit(uint32_t bits16, uint32_t lo0, uint32_t lo1, uint32_t hi, const float* sq, uint32_t d0,
                                        bf_f2 (&bd)[kBfQ / 2], bf_f2 (&ed)[kBfQ / 2]) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        // MSB-first: dimension j of the unit is bit 7 - (j % 8) of byte j / 8 (bits16 = byte0 | byte1 << 8)
        const float b = (float)((bits16 >> ((j < 8 ? 0 : 8) + 7 - (j & 7))) & 1u);
        const bf_f2 b2 = {b, b};
        const float4* qrow = reinterpret_cast<const float4*>(sq + (size_t)(d0 + j) * kBfQ);
        if (EX == 0) {
#pragma unroll
            for (uint32_t t = 0; t < kBfQ / 4; ++t) {
                const float4 q = qrow[t];
                const bf_f2 qa = {q.x, q.y}, qb = {q.z, q.w};
                bd[2 * t] = bd[2 * t] + b2 * qa;
                bd[2 * t + 1] = bd[2 * t + 1] + b2 * qb;
            }
        } else {
            const float c = bf_ex_code<EX>(lo0, lo1, hi, j);
            const bf_f2 c2 = {c, c};
#pragma unroll
            for (uint32_t t = 0; t < kBfQ / 4; ++t) {
                const float4 q = qrow[t];
                const bf_f2 qa = {q.x, q.y}, qb = {q.z, q.w};
                bd[2 * t] = bd[2 * t] + b2 * qa;
                bd[2 * t + 1] = bd[2 * t + 1] + b2 * qb;
                ed[2 * t] = ed[2 * t] + c2 * qa;
                ed[2 * t + 1] = ed[2 * t + 1] + c2 * qb;
            }
        }
        // keeps the scheduler from hoisting the LDS reads of all 16 dimensions above the first one's arithmetic (462 VGPRs at
        // 6 bits without it: one wave per SIMD)
        asm volatile("" ::: "memory");
    }
}

// grid: (ceil(nv / kBfVec), ceil(nq / kBfQ)); block kBfVec; static LDS kBfChunk x kBfQ floats
template <int EX>
__global__ __launch_bounds__(kBfVec) void k_bf_dist(BfDistParams P) {
    __shared__ __attribute__((aligned(16))) float sq[kBfChunk * kBfQ];
    const uint32_t tid = threadIdx.x;
    const uint64_t vl = (uint64_t)blockIdx.x * kBfVec + tid;       // vector inside the chunk
    const uint64_t v = P.v0 + vl;                                   // vector id
    const bool live = vl < P.nv;
    const uint32_t q0 = blockIdx.y * kBfQ;
    const uint32_t D = P.D;
    const uint32_t bin_row = D / 8, ex_row = D * EX / 8;
    const uint8_t* bin = P.bin + (live ? v : 0) * bin_row;
    const uint8_t* exc = EX ? P.ex + (live ? v : 0) * ex_row : nullptr;
    bf_f2 bd[kBfQ / 2], ed[kBfQ / 2];
#pragma unroll
    for (uint32_t t = 0; t < kBfQ / 2; ++t) { bd[t] = (bf_f2){0.0f, 0.0f}; ed[t] = (bf_f2){0.0f, 0.0f}; }
    for (uint32_t c0 = 0; c0 < D; c0 += kBfChunk) {
        const uint32_t cn = D - c0 < kBfChunk ? D - c0 : kBfChunk; // multiple of 16 (D % 16 == 0)
        __syncthreads();
        for (uint32_t e = tid; e < kBfChunk * kBfQ; e += kBfVec) {
            const uint32_t j = e % kBfQ, i = e / kBfQ;
            const uint32_t q = q0 + j;
            sq[e] = (q < P.nq && i < cn) ? P.rot[(size_t)q * D + c0 + i] : 0.0f;
        }
        __syncthreads();
        for (uint32_t u = 0; u < cn; u += 16) {
            const uint32_t dim0 = c0 + u;
            const uint32_t bits16 = (uint32_t)bin[dim0 / 8] | ((uint32_t)bin[dim0 / 8 + 1] << 8);
            uint32_t lo0 = 0, lo1 = 0, hi = 0;
            if (EX == 6) {
                const uint32_t* p = reinterpret_cast<const uint32_t*>(exc + (size_t)dim0 / 16 * 12); // 4-byte aligned: D/16*12 per row
                lo0 = p[0]; lo1 = p[1]; hi = p[2];
            } else if (EX == 2) {
                hi = *reinterpret_cast<const uint32_t*>(exc + (size_t)dim0 / 16 * 4);
            }
            bf_unit<EX>(bits16, lo0, lo1, hi, sq, u, bd, ed);
        }
    }
    if (!live) return;
    bool pass = true;
    if (P.filter) pass = v < P.filter_nbits && ((P.filter[v >> 5] >> (v & 31u)) & 1u);
    const float f_add = EX ? P.f_add_ex[v] : P.f_add[v];
    const float f_res = EX ? P.f_rescale_ex[v] : P.f_rescale[v];
#pragma unroll
    for (uint32_t j = 0; j < kBfQ; ++j) {
        const uint32_t q = q0 + j;
        if (q >= P.nq) break;
        const QueryConsts& qc = P.consts[q];
        const float b = (j & 1u) ? bd[j / 2].y : bd[j / 2].x;
        float dist;
        if (EX == 0) {
            const float t = b + qc.k1x;
            dist = (f_add + 0.0f) + f_res * t;
        } else {
            const float e = (j & 1u) ? ed[j / 2].y : ed[j / 2].x;
            const float t = ((qc.scale * b) + e) + qc.kbx;
            dist = (f_add + 0.0f) + f_res * t;
        }
        P.dist[(size_t)q * P.nv + vl] = pass ? dist : __int_as_float(0x7fc00000);
    }
}

// Rust BinaryHeap state of one query that spans several vector chunks: heap_d / heap_s [nq][top_k + 1], heap_len [nq]
// grid: nq; block 64 (one wave); dynamic LDS (top_k + 1) * 8 bytes when the heap lives in LDS (P.lds_heap), else 0.
__global__ __launch_bounds__(64) void k_bf_select(BfSelectParams P) {
    extern __shared__ __attribute__((aligned(16))) uint32_t bf_lds[];
    const uint32_t q = blockIdx.x, lane = threadIdx.x, K = P.top_k;
    float* gd = P.heap_d + (size_t)q * (K + 1);
    uint32_t* gs = P.heap_s + (size_t)q * (K + 1);
    float* hd = P.lds_heap ? reinterpret_cast<float*>(bf_lds) : gd;
    uint32_t* hs = P.lds_heap ? bf_lds + (K + 1) : gs;
    uint32_t len = P.first ? 0u : P.heap_len[q];
    if (P.lds_heap && !P.first)
        for (uint32_t i = lane; i < len; i += 64) { hd[i] = gd[i]; hs[i] = gs[i]; }
    __syncthreads();
    LdsHeap h{hd, hs, len};
    // Skipping: once the heap is full, the reference's push of a key above the root followed by its pop leaves the array as it
    // was (topk.hpp, tie_log_replay: the key climbs the path from slot top_k to the root and the pop walks back down the same
    // path) unless some node of that path equals its off-path child.  `ptie` is that condition, re-evaluated after every real
    // insertion; while it is false such a candidate is skipped.  Keys equal to the root are never skipped.
    auto path_tie = [&]() -> bool {
        bool t = false;
        for (uint32_t c = K; c > 0;) {
            const uint32_t par = (c - 1u) >> 1, sib = (c & 1u) ? c + 1u : c - 1u;
            if (sib < K) t |= __float_as_int(hd[par]) == __float_as_int(hd[sib]);
            c = par;
        }
        return t;
    };
    bool ptie = h.len == K ? path_tie() : false;
    const float* row = P.dist + (size_t)q * P.nv;
    uint32_t n_push = 0, n_tie = 0;
    // the row is read kBfSelU groups of 64 at a time, all loads in flight before the first group is decided (one memory round trip
    // per 64 * kBfSelU distances instead of one per 64)
    constexpr uint32_t kBfSelU = 8;
    for (uint64_t s0 = 0; s0 < P.nv; s0 += 64 * kBfSelU) {
        float dv[kBfSelU];
#pragma unroll
        for (uint32_t u = 0; u < kBfSelU; ++u) {
            const uint64_t i = s0 + 64 * u + lane;
            dv[u] = i < P.nv ? row[i] : __int_as_float(0x7fc00000);
        }
#pragma unroll
        for (uint32_t u = 0; u < kBfSelU; ++u) {
            const uint64_t b0 = s0 + 64 * u;
            const float d = dv[u];
            const bool fin = finite_f(d);
            const int32_t kd = total_key(d);
            uint64_t done = 0; // lanes of this group already decided
            while (true) {
                const bool full = h.len == K;
                const int32_t rk = full ? total_key(hd[0]) : 0;
                const bool cand = fin && (!full || kd <= rk || ptie) && !((done >> lane) & 1ull);
                const uint64_t m = __ballot(cand);
                if (!m) break;
                const uint32_t j = (uint32_t)__builtin_ctzll(m);
                done = j == 63 ? ~0ull : ((2ull << j) - 1ull);
                const float dj = __shfl(d, (int)j);
                if (full && (total_key(dj) == rk || ptie)) ++n_tie;
                ++n_push;
                if (lane == 0) {
                    h.push(dj, (uint32_t)(P.v0 + b0 + j));
                    if (h.len > K) h.pop();
                } else {
                    h.len = h.len + 1u > K ? K : h.len + 1u;
                }
                __syncthreads();
                ptie = h.len == K ? path_tie() : false;
            }
        }
    }
    if (lane == 0 && n_push) { atomicAdd(P.stats, (unsigned long long)n_push); if (n_tie) atomicAdd(P.stats + 1, (unsigned long long)n_tie); }
    if (!P.last) {
        if (P.lds_heap)
            for (uint32_t i = lane; i < h.len; i += 64) { gd[i] = hd[i]; gs[i] = hs[i]; }
        if (lane == 0) P.heap_len[q] = h.len;
        return;
    }
    // into_sorted_vec, then the stable sort by distance (L2) / by score = -distance descending (IP): negation reverses the
    // total order, so both leave into_sorted_vec's ascending order as it is
    if (lane == 0) h.into_sorted();
    __syncthreads();
    uint64_t* oid = P.out_ids + (size_t)q * K;
    float* osc = P.out_scores + (size_t)q * K;
    for (uint32_t i = lane; i < K; i += 64) {
        if (i < h.len) {
            const float d = hd[i];
            oid[i] = hs[i];
            osc[i] = P.metric == 0 ? d : -d;
        } else {
            oid[i] = ~0ull;
            osc[i] = __int_as_float(0x7fc00000);
        }
    }
    if (lane == 0) P.out_counts[q] = h.len;
}

} // namespace rbq
