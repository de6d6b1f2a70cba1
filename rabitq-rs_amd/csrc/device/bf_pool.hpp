// bf_pool.hpp — kernels of the ranked rerank pool on brute-force handles (rbq_bf_search_exact_ranked_batch,
// include/ext/rbq_bf_range.h): per query the P = max(pool, top_k) best estimates by the key
// (f32::total_cmp order of the distance, id ascending), found by a radix select instead of k_bf_select's heap replay.  They run
// behind k_bf_dist (bf.hpp) on the [nq][nv] f32 workspace of a (query sub-batch, vector chunk), NaN for a filtered-out vector,
// and hand k_bf_rerank_score / k_bf_rerank_order (bf_rerank.hpp) the pool's ids and counts.
//
// A query's row is cut into the spans of the range search (kBfRangeSpan vectors, bf_range_span.hpp); one workgroup of 256 threads
// owns a (block, query).  Block b >= n_carry is span b - n_carry of the chunk; blocks 0 .. n_carry - 1 (none on a call's first
// chunk) cover the query's pool so far, at most P packed entries `key << 32 | id` carried from the earlier chunks, whose ids are
// all smaller: they take part in every step as spans ahead of span 0.  The key of a distance d is
// (uint32_t)total_key(d) ^ 0x80000000u, ascending as total_cmp; a non-finite d is no candidate and gets kBfPoolNoKey, which is
// above every candidate's key.
//
//   k_bf_pool_hist, pass p = 0 .. 3   the state after pass p - 1 — the key's digits so far and the rank wanted among the keys
//                     that share them — comes from the query's global histogram of pass p - 1, reduced by every workgroup of the
//                     query for itself (bf_pool_state).  The block's candidates that match the digits so far are counted by
//                     their next 8-bit digit in LDS, and the non-zero bins are added to the query's histogram of pass p with
//                     integer atomicAdd: sums that do not depend on the order of arrival.
//   k_bf_pool_count   the state after pass 3 is T, the P-th smallest key, and `need`, the keys equal to T to take.  Each block
//                     writes two counts: its keys below T and its keys equal to T.
//   k_bf_pool_place   sums the counts of the earlier blocks and of all blocks.  An entry below T goes to its rank among the
//                     entries below T in block order; an entry equal to T whose rank r among those, in the same order, is below
//                     `need` goes to (entries below T) + r.  Block order is id order, so the smallest ids win the ties, and entries
//                     of equal key stay in ascending id order in the list, which is what the next chunk's placement relies on.
//                     On the last chunk the ids go to the rerank kernels' rows, else the packed entries to the other carried list.
//
// Fewer candidates than P: the state's rank becomes 0, T = kBfPoolNoKey, and every candidate is below T.  Every position is a sum
// of counts written by an earlier launch or by the workgroup itself: no atomic decides a position, no workgroup waits on another.
// No floating-point arithmetic: compares and bit maps only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "launch.hpp"
#include "bf_range_span.hpp" // kBfRangeThreads / Rounds / Waves, bf_range_load

namespace rbq {

constexpr uint32_t kBfPoolNoKey = 0xffffffffu; // (the key of the largest finite f32 is 0xff7fffff)
static_assert(kBfPoolBins == kBfRangeThreads && kBfRangeThreads == (uint32_t)kThreads, "one thread per bin; block_scan_excl256");
static_assert(kBfPoolPasses * kBfPoolDigitBits == 32u, "the passes cover the key");

__device__ __forceinline__ uint32_t bf_pool_key(float d) { return finite_f(d) ? (uint32_t)total_key(d) ^ 0x80000000u : kBfPoolNoKey; }

// the lane's kBfRangeRounds keys (and, IDS, ids) of block blk, in the rounds' order: entry kBfRangeThreads * u + tid of the block
template <bool IDS>
__device__ __forceinline__ void bf_pool_load(const BfPoolParams& P, uint32_t q, uint32_t blk, uint32_t tid, uint32_t (&key)[kBfRangeRounds],
                                             uint32_t (&id)[kBfRangeRounds]) {
    if (blk < P.n_carry) { // (the whole workgroup)
        const unsigned long long* row = P.carry_in + (size_t)q * P.pool;
        const uint32_t n = min(P.carry_n_in[q], P.pool);
#pragma unroll
        for (uint32_t u = 0; u < kBfRangeRounds; ++u) {
            const uint32_t i = blk * kBfRangeSpan + kBfRangeThreads * u + tid;
            const unsigned long long e = i < n ? row[i] : ~0ull;
            key[u] = (uint32_t)(e >> 32);
            if (IDS) id[u] = (uint32_t)e;
        }
    } else {
        const uint32_t span = blk - P.n_carry;
        float dv[kBfRangeRounds];
        bf_range_load(P, q, span, tid, dv);
#pragma unroll
        for (uint32_t u = 0; u < kBfRangeRounds; ++u) {
            key[u] = bf_pool_key(dv[u]);
            if (IDS) id[u] = (uint32_t)(P.v0 + (uint64_t)span * kBfRangeSpan + kBfRangeThreads * u + tid); // (an id is below 2^32)
        }
    }
}

// The select state of query q after `pass` passes, the same in every thread: x = the key's top 8 * pass bits, y = the rank wanted
// (1-based) among the candidates that share them; y == 0: fewer candidates than the pool, x = kBfPoolNoKey.  It is the state after
// pass - 1 passes (P.state, written by block 0 of the launch before; none before pass 1) moved on by the histogram of pass - 1.
// The whole workgroup calls it; s_w: 4 words, s_st: 2 words of LDS; a barrier stands between the last LDS access and the return.
__device__ __forceinline__ uint2 bf_pool_state(const BfPoolParams& P, uint32_t q, uint32_t pass, uint32_t tid, uint32_t* s_w, uint32_t* s_st) {
    uint2 st = make_uint2(0u, P.pool);
    if (pass > 1u) st = make_uint2(P.state[((size_t)(pass - 1u) * P.nq + q) * 2u], P.state[((size_t)(pass - 1u) * P.nq + q) * 2u + 1u]);
    if (pass == 0u || st.y == 0u) { // (uniform)
        __syncthreads();
        return pass ? make_uint2(kBfPoolNoKey, 0u) : st;
    }
    const uint32_t c = P.hist[((size_t)(pass - 1u) * P.nq + q) * kBfPoolBins + tid];
    uint32_t total;
    const uint32_t excl = block_scan_excl256(c, s_w, tid, total);
    if (excl < st.y && st.y <= excl + c) { // the one bin that holds the rank
        s_st[0] = st.x | tid << (32u - kBfPoolDigitBits * pass);
        s_st[1] = st.y - excl;
    }
    if (tid == 0u && total < st.y) { // (pass 1 only: a later histogram holds at least the rank it was entered with)
        s_st[0] = kBfPoolNoKey;
        s_st[1] = 0u;
    }
    __syncthreads();
    return make_uint2(s_st[0], s_st[1]);
}

__device__ __forceinline__ void bf_pool_state_store(const BfPoolParams& P, uint32_t q, uint32_t pass, uint2 st) {
    P.state[((size_t)pass * P.nq + q) * 2u] = st.x;
    P.state[((size_t)pass * P.nq + q) * 2u + 1u] = st.y;
}

// grid: (n_carry + n_spans, nq); block kBfRangeThreads
__global__ __launch_bounds__(kBfRangeThreads) void k_bf_pool_hist(BfPoolParams P, uint32_t pass) {
    __shared__ uint32_t s_hist[kBfPoolBins];
    __shared__ uint32_t s_w[kBfRangeWaves], s_st[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, blk = blockIdx.x, q = blockIdx.y;
    uint32_t key[kBfRangeRounds], id[kBfRangeRounds];
    bf_pool_load<false>(P, q, blk, tid, key, id); // in flight under the reduction below
    s_hist[tid] = 0u;
    const uint2 st = bf_pool_state(P, q, pass, tid, s_w, s_st);
    if (pass && blk == 0u && tid == 0u) bf_pool_state_store(P, q, pass, st);
    if (st.y == 0u) return; // (the whole workgroup) every candidate is taken: nothing left to find

    const uint32_t shift = 32u - kBfPoolDigitBits * (pass + 1u);
#pragma unroll
    for (uint32_t u = 0; u < kBfRangeRounds; ++u) {
        // a candidate that shares the digits so far ((key ^ x) >> 32 is no shift: pass 0 takes every candidate)
        bool in = key[u] != kBfPoolNoKey && (pass == 0u || ((key[u] ^ st.x) >> (shift + kBfPoolDigitBits)) == 0u);
        const uint32_t digit = (key[u] >> shift) & (kBfPoolBins - 1u);
        // The leading digits of a query's distances are nearly all alike: the lanes that share the digit of the wave's first
        // candidate are counted by one ballot and added once, twice over; what is left adds for itself.
#pragma unroll
        for (uint32_t r = 0; r < 2u; ++r) {
            const uint64_t todo = __ballot(in);
            if (todo == 0ull) break; // (wave-uniform)
            const uint32_t lead = (uint32_t)__builtin_amdgcn_readlane((int)digit, (int)__builtin_ctzll(todo));
            const bool mine = in && digit == lead;
            const uint32_t cnt = (uint32_t)__popcll(__ballot(mine));
            if (lane == 0u) atomicAdd(&s_hist[lead], cnt);
            in = in && !mine;
        }
        if (in) atomicAdd(&s_hist[digit], 1u);
    }
    __syncthreads();
    const uint32_t c = s_hist[tid];
    if (c) atomicAdd(&P.hist[((size_t)pass * P.nq + q) * kBfPoolBins + tid], c);
}

// grid: (n_carry + n_spans, nq); block kBfRangeThreads
__global__ __launch_bounds__(kBfRangeThreads) void k_bf_pool_count(BfPoolParams P) {
    __shared__ uint32_t s_w[kBfRangeWaves], s_st[2];
    __shared__ uint32_t s_c[2][kBfRangeWaves];
    const uint32_t tid = threadIdx.x, blk = blockIdx.x, q = blockIdx.y;
    uint32_t key[kBfRangeRounds], id[kBfRangeRounds];
    bf_pool_load<false>(P, q, blk, tid, key, id);
    const uint2 st = bf_pool_state(P, q, kBfPoolPasses, tid, s_w, s_st); // x = T, y = need
    if (blk == 0u && tid == 0u) bf_pool_state_store(P, q, kBfPoolPasses, st);
    uint32_t less = 0, eq = 0; // wave-uniform
#pragma unroll
    for (uint32_t u = 0; u < kBfRangeRounds; ++u) {
        less += (uint32_t)__popcll(__ballot(key[u] < st.x));
        eq += (uint32_t)__popcll(__ballot(key[u] == st.x && key[u] != kBfPoolNoKey));
    }
    if ((tid & 63u) == 0u) { s_c[0][tid >> 6] = less; s_c[1][tid >> 6] = eq; }
    __syncthreads();
    if (tid < 2u) {
        uint32_t t = 0;
#pragma unroll
        for (uint32_t w = 0; w < kBfRangeWaves; ++w) t += s_c[tid][w];
        const uint32_t nb = P.n_carry + P.n_spans;
        P.span_counts[((size_t)tid * P.nq + q) * nb + blk] = t; // [0]: below T, [1]: equal to T
    }
}

// grid: (n_carry + n_spans, nq); block kBfRangeThreads
__global__ __launch_bounds__(kBfRangeThreads) void k_bf_pool_place(BfPoolParams P) {
    __shared__ uint32_t s_sum[4][kBfRangeWaves];
    __shared__ uint32_t s_cnt[2][kBfRangeRounds][kBfRangeWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, blk = blockIdx.x, q = blockIdx.y;
    const uint32_t nb = P.n_carry + P.n_spans;
    uint32_t key[kBfRangeRounds], id[kBfRangeRounds];
    bf_pool_load<true>(P, q, blk, tid, key, id); // in flight under the reduction below
    const uint32_t T = P.state[((size_t)kBfPoolPasses * P.nq + q) * 2u], need = P.state[((size_t)kBfPoolPasses * P.nq + q) * 2u + 1u];

    // entries below T and equal to T: of the blocks before this one, and of all blocks
    const uint32_t* cl = P.span_counts + (size_t)q * nb;
    const uint32_t* ce = P.span_counts + ((size_t)P.nq + q) * nb;
    uint32_t sums[4] = {0u, 0u, 0u, 0u};
    for (uint32_t j = tid; j < nb; j += kBfRangeThreads) {
        const uint32_t a = cl[j], b = ce[j];
        sums[0] += j < blk ? a : 0u;
        sums[1] += a;
        sums[2] += j < blk ? b : 0u;
        sums[3] += b;
    }
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        sums[k] = wave_sum_u32(sums[k]);
        if (lane == 0u) s_sum[k][wave] = sums[k];
    }
    uint64_t bal[2][kBfRangeRounds]; // wave-uniform
#pragma unroll
    for (uint32_t u = 0; u < kBfRangeRounds; ++u) {
        bal[0][u] = __ballot(key[u] < T);
        bal[1][u] = __ballot(key[u] == T && key[u] != kBfPoolNoKey);
        if (lane == 0u) { s_cnt[0][u][wave] = (uint32_t)__popcll(bal[0][u]); s_cnt[1][u][wave] = (uint32_t)__popcll(bal[1][u]); }
    }
    __syncthreads();
    uint32_t tot[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t w = 0; w < kBfRangeWaves; ++w)
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) tot[k] += s_sum[k][w];
    const uint32_t n_less = tot[1], taken = n_less + min(need, tot[3]); // the query's pool after this chunk
    if (tid == 0u && blk + 1u == nb) {
        if (P.last) P.out_counts[q] = min(taken, P.pool);
        else P.carry_n_out[q] = min(taken, P.pool);
    }

    uint32_t pos[2] = {tot[0], tot[2]}; // rank of the round's first entry among the entries below T / equal to T
#pragma unroll
    for (uint32_t u = 0; u < kBfRangeRounds; ++u) {
        uint32_t p = P.pool; // (no slot)
#pragma unroll
        for (uint32_t k = 0; k < 2u; ++k) {
            uint32_t lower = 0, round = 0;
#pragma unroll
            for (uint32_t w = 0; w < kBfRangeWaves; ++w) {
                const uint32_t c = s_cnt[k][u][w];
                lower += w < wave ? c : 0u;
                round += c;
            }
            const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal[k][u] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal[k][u], 0u));
            const uint32_t r = pos[k] + lower + below;
            if ((bal[k][u] >> lane) & 1ull) p = k == 0u ? r : (r < need ? n_less + r : P.pool);
            pos[k] += round;
        }
        if (p < P.pool) { // (n_less + need <= pool: the bound only guards the row)
            if (P.last) P.out_ids[(size_t)q * P.pool + p] = id[u];
            else P.carry_out[(size_t)q * P.pool + p] = ((unsigned long long)key[u] << 32) | id[u];
        }
    }
}

} // namespace rbq
