// scan.hpp — k_scan, the roofline kernel of the IVF+RaBitQ query path (gfx950, wave64).
//
// Reference semantics: search_cluster_v2_batched (src/ivf.rs:1901-2129) over the probed lists of one
// query, i.e. accumulate_batch (src/simd.rs:972-1184) + compute_batch_distances_u16 (:2090-2140) +
// lower-bound pruning + ip_packed_ex{2,6}_f32 (:1835-1915) + BinaryHeap top-k (src/ivf.rs:904-931).
//
// One workgroup = one query, with fixed wave roles:
//   waves 0..NS-1 "scanners": consume the query's block stream (k_select_mfma: probe order, block order inside a
//             list, each entry with its precomputed block-level lower bound) in fill steps (one lane per entry:
//             bound vs threshold -> live-block FIFO) and tile steps (2*NS live blocks, lane = vector: codes ->
//             LDS LUT lookups -> fused epilogue); survivors (lb < T) are published (mask, lb, ip, est, slot) to a
//             double-buffered LDS queue.
//   wave NS   "replay wave": compacts the previous tile's survivors in stream order, refines lazily (only
//             survivors still below the true threshold, 16 lanes per survivor over a lane-major copy of the ex
//             codes) and replays them through the reference's exact prune/push/pop loop while the scanners are
//             already on the next tile; publishes T.  The top-k lives in the wave's registers: a sorted run while
//             all distances are distinct, the Rust-BinaryHeap-faithful RegHeap after an in-kernel restart
//             otherwise (see SortedTop).
// Exactness: scanners prune with a STALE threshold T.  T only ever shrinks, so `lb >= T_stale` implies the
// reference (whose threshold at that moment is <= T_stale) skipped the candidate too; everything else is
// re-tested by the replay wave against the true running threshold, in stream order.  ids therefore equal
// the sequential CPU path bit for bit.  Tiles with more than kLightMax survivors (the first probed lists,
// where T is still loose) run synchronously, software-pipelined: the scanners' groups refine batch r+1 while
// the replay wave replays batch r.
#pragma once
#include "kernels.hpp"
#include "scan_codes.hpp"
#include "topk.hpp"

namespace rbq {

#ifndef RBQ_SCAN_WAVES
#define RBQ_SCAN_WAVES 5    // launch-bounds occupancy target (waves per SIMD): 96 VGPRs, room for a fifth wave of another kernel
#endif
#ifndef RBQ_LIGHT_MAX
#define RBQ_LIGHT_MAX 12
#endif
constexpr uint32_t kLightMax = RBQ_LIGHT_MAX;   // tiles with more survivors than this run synchronously
constexpr uint32_t kBatchDone = 0xffffffffu;

constexpr uint32_t kWinGrow = 4;                // growth of the fill window per step
// EX: compile-time ex_bits (0/2/6) when DT != 0; ignored (runtime P.ex_bits) when DT == 0.
// TR: registers per lane of the replay wave's top-k (1: top_k <= 63; 2: <= 128; 4: <= 256 — with more than one,
// four waves per SIMD instead of five).
// V: numeric variant (kernels.hpp, kVarAvx512 / kVarAvx2 / kVarPortable).  The variants other than the default are instantiated
// for the runtime-dimension kernel only (DT = 0), so the default instantiations keep their code and the build its size.
template <int DT, int EX, int TR, int V = kVarAvx512>
__global__ __launch_bounds__(kScanThreads, ((TR == 1 && scan_nb((uint32_t)DT) == 1) ? RBQ_SCAN_WAVES : 4)) void k_scan(ScanParams P) {
    extern __shared__ __align__(16) unsigned char smraw[];
    // blocks per scanner half-wave and tile: 1; a build option gives 2 at small dimensions (types.hpp: measured, not faster)
    constexpr int NB = scan_nb((uint32_t)DT);
    constexpr int kTB = kTileBlocks * NB;  // blocks per tile
    constexpr int kTC = kTileCand * NB;    // candidates per tile
    const uint32_t Dc = DT ? (uint32_t)DT : P.Dc; // code/LUT dimension (x64)
    const uint32_t D = DT ? (uint32_t)DT : P.D;   // padded_dim (ex codes, rotated query)
    uint8_t* s_lut = smraw;
    float* s_q = reinterpret_cast<float*>(smraw + (size_t)Dc * 4);
    // the exact heap of top_k + 1 entries: in LDS, or (top_k beyond the LDS: the reference accepts any top_k, src/ivf.rs:2116-2126)
    // in this query's slice of a global workspace — one lane works on it either way
    const uint32_t hk = P.heap_ws ? 0u : P.top_k + 1u;
    float* heap_d = s_q + ex_qlen(D, DT ? (uint32_t)EX : P.ex_bits);
    uint32_t* heap_s = reinterpret_cast<uint32_t*>(heap_d + hk);
    uint32_t* q_slot = heap_s + hk;                      // [2][kTileCand]
    if (P.heap_ws) {
        heap_d = reinterpret_cast<float*>(P.heap_ws + (size_t)blockIdx.x * 2 * ((size_t)P.top_k + 1));
        heap_s = reinterpret_cast<uint32_t*>(heap_d + (P.top_k + 1));
    }
    float* q_lb = reinterpret_cast<float*>(q_slot + 2 * kTC);
    float* q_ip = q_lb + 2 * kTC;
    float* q_gadd = q_ip + 2 * kTC;
    float* q_d = q_gadd + 2 * kTC;
    uint32_t* s_list = reinterpret_cast<uint32_t*>(q_d + 2 * kTC); // [kTC] survivor positions, stream order
    uint32_t* s_mask = s_list + kTC;                                // [2][kTB]
    WorkItem* s_queue = reinterpret_cast<WorkItem*>(s_mask + 2 * kTB); // [kQueueCap] live blocks, stream order
    unsigned long long* s_fmask = reinterpret_cast<unsigned long long*>(s_queue + kQueueCap); // [kFillK][kNScan] fill-step live masks
    // no static __shared__ in this kernel: the dynamic region must start at LDS address 0 (see lds_lut_ptr)
    uint32_t* s_misc = reinterpret_cast<uint32_t*>(s_fmask + kNScan * kFillK);
    float& s_T = *reinterpret_cast<float*>(s_misc);
    uint32_t& s_len = *(s_misc + 1);
    uint32_t* s_nskip = s_misc + 2;
    uint32_t& s_nbatch = *(s_misc + 3);   // refine batch size of the current round (kBatchDone = tile finished)
    uint32_t& s_restart = *(s_misc + 4);  // a distance tie was met on the sorted fast path: re-run with the exact heap
    uint32_t* s_batch = s_misc + 8;       // [2*kScanThreads/16] queue positions to refine in this round

    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t wave = tid >> 6, lane = tid & 63u, half = lane >> 5, l32 = lane & 31u;
    const uint32_t hw = tid >> 5; // half-wave index; scanners own blocks 0..kTileBlocks-1 of a tile
    const bool scanner = wave < (uint32_t)kNScan;
    const lds_lut_ptr lut0 = (lds_lut_ptr)(uint32_t)0; // == s_lut
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smraw != 0u) __builtin_trap();
    const uint32_t top_k = P.top_k;
    const uint32_t ex_bits = DT ? (uint32_t)EX : P.ex_bits;
    const size_t stride = (size_t)Dc * 4 + 384;
    const size_t exb = ex_bytes_dev(D, ex_bits);
    const uint32_t nunits = ex_w4(D, ex_bits), qlen = ex_qlen(D, ex_bits);

    {
        const uint4* src = reinterpret_cast<const uint4*>(P.lut + (size_t)q * Dc * 4);
        uint4* dst = reinterpret_cast<uint4*>(s_lut);
        for (uint32_t i = tid; i < Dc / 4; i += kScanThreads) dst[i] = src[i];
        // (the rotated query as 16-byte loads, all of a thread's in flight before its first LDS store: the plain dword loop waited for
        // every load in front of its ds_write — four dependent round trips at D = 960 before the first fill step)
        const float4* rs = reinterpret_cast<const float4*>(P.rot + (size_t)q * D); // (D % 4 == 0: padded_dim is a multiple of 64)
        float4* rd = reinterpret_cast<float4*>(s_q);
        for (uint32_t i0 = tid; i0 < qlen / 4; i0 += 2 * kScanThreads) {
            float4 b[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) { const uint32_t i = i0 + (uint32_t)u * kScanThreads; b[u] = (i < qlen / 4 && i < D / 4) ? rs[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
#pragma unroll
            for (int u = 0; u < 2; ++u) { const uint32_t i = i0 + (uint32_t)u * kScanThreads; if (i < qlen / 4) rd[i] = b[u]; }
        }
        if (tid == 0) { s_T = INFINITY; *s_nskip = 0; s_len = 0; s_restart = 0; s_misc[5] = 0; s_misc[6] = 0; s_misc[7] = 0; }
    }
    // the replay wave is the serial part of every tile: let it issue ahead of the (many) scanner waves it shares
    // its SIMD with
    if (!scanner) __builtin_amdgcn_s_setprio(3);
    const QueryConsts qc = P.consts[q];
    const ProbeInfo* probe = P.probe + (size_t)q * P.nprobe;
    const StreamItem* wl = P.wl + (size_t)q * P.wl_stride;
    const uint32_t ns = P.nstream[q];
    __syncthreads();

    uint32_t n_skip = 0, n_ext = 0, n_est = 0; // n_skip: every thread; n_ext/n_est: replay wave (uniform)
    // traffic counters of an open profile (P.prof): block records whose codes / factor rows this half-wave
    // requested, passes over the stream, ex-code evaluations (they survive an exact-heap restart: the traffic is real)
    uint32_t p_code = 0, p_meta = 0, p_pass = 1; // (candidates whose ex codes were fetched are counted in s_misc[7])
    const bool count_skips = P.diag != nullptr;

    bool fast = top_k <= 64u * TR && !P.exact_heap && !P.mstg; // sorted run (SortedRun / RankRun) until a distance tie shows up
    uint32_t* const tlog = P.tie_log ? P.tie_log + (size_t)q * P.tie_log_cap * 3u : nullptr; // tie log of this query (see `log_n` below)
    // group `g` (16 lanes) refines the survivor at queue position s_batch[g] of tile buffer `buf`.  The ex
    // factors are requested together with the code units, not after the dot product.
    auto refine_batch = [&](uint32_t buf, uint32_t nb, uint32_t g) {
        const uint32_t gl = tid & 15u;
        if (g < nb) {
            const uint32_t e = buf * kTC + s_batch[g];
            const uint32_t sl = q_slot[e];
            const uint8_t* ex = P.ex_codes + (size_t)sl * exb;
            float sacc;
            float fa, fr;
            if constexpr (V != kVarAvx512) {
                fa = P.f_add_ex[sl]; fr = P.f_rescale_ex[sl];
                sacc = ex_dot_var_rt<V>(ex, s_q, gl, nunits, D / 16, ex_bits); // (already the group's sum)
            } else if (nunits <= (uint32_t)kExRegUnits) {
                uint4 u[kExRegUnits];
                ex_load_all(u, ex, gl, nunits);
                fa = P.f_add_ex[sl]; fr = P.f_rescale_ex[sl];
                asm volatile("" : "+v"(fa), "+v"(fr)); // issue the loads here
                sacc = ex_bits == 6 ? ex_dot_all<6>(u, s_q, gl, nunits) : ex_dot_all<2>(u, s_q, gl, nunits);
            } else {
                fa = P.f_add_ex[sl]; fr = P.f_rescale_ex[sl];
                asm volatile("" : "+v"(fa), "+v"(fr));
                sacc = ex_bits == 6 ? ex_dot_units<6>(ex, s_q, gl, nunits) : ex_dot_units<2>(ex, s_q, gl, nunits);
            }
            if constexpr (V == kVarAvx512) sacc = group16_reduce(sacc);
            if (gl == 0) q_d[e] = refined_distance(qc.scale, q_ip[e], sacc, qc.kbx, fa, q_gadd[e], fr);
        }
    };

    // small dimensions (one code unit per lane): group `g` of `ng` refines the survivors at queue positions
    // s_batch[g] and s_batch[g + ng] in one pass
    // (heavy tiles, a vector's codes spanning several units: two survivors per 16-lane group and round, one after the other, halve the
    // rounds of barrier + collect + replay at the price of a larger superset — measured: slower, scan 0.139-0.144 against 0.135-0.139 ms)
    constexpr uint32_t kNU = ex_w4((uint32_t)(DT ? DT : 16), (uint32_t)(EX ? EX : 2)); // code units per lane and vector
    constexpr bool kDual1 = DT != 0 && EX != 0 && kNU == 1u;
    constexpr bool kDualN = DT != 0 && EX != 0 && TR > 1 && kNU >= 2u && kNU <= 3u; // packed pair refine (top_k >= 64)
    constexpr bool kDual = kDual1 || kDualN;
    auto refine_pair = [&](uint32_t buf, uint32_t nb, uint32_t g, uint32_t ng) {
        const uint32_t gl = tid & 15u;
        if (g >= nb) return;
        const bool has1 = g + ng < nb;
        const uint32_t e0 = buf * kTC + s_batch[g];
        const uint32_t e1 = buf * kTC + s_batch[has1 ? g + ng : g];
        const uint32_t sl0 = q_slot[e0], sl1 = q_slot[e1];
        const uint4* p0 = reinterpret_cast<const uint4*>(P.ex_codes + (size_t)sl0 * exb) + gl;
        const uint4* p1 = reinterpret_cast<const uint4*>(P.ex_codes + (size_t)sl1 * exb) + gl;
        // (no register pin on the four factor loads: it made the wave WAIT for them before the code units were even requested)
        const float fa0 = P.f_add_ex[sl0], fr0 = P.f_rescale_ex[sl0], fa1 = P.f_add_ex[sl1], fr1 = P.f_rescale_ex[sl1];
        float sa, sb;
        if constexpr (V != kVarAvx512) { // (not reached: the variants are DT = 0 instantiations, which never pair)
            sa = ex_dot_var_rt<V>(P.ex_codes + (size_t)sl0 * exb, s_q, gl, nunits, D / 16, ex_bits);
            sb = ex_dot_var_rt<V>(P.ex_codes + (size_t)sl1 * exb, s_q, gl, nunits, D / 16, ex_bits);
        } else if (kDualN) ex_dot_pair_all<(EX ? EX : 2), (kDualN ? (int)kNU : 1)>(p0, p1, s_q, gl, sa, sb);
        else {
            const uint4 u0 = p0[0], u1 = p1[0];
            if (EX == 6) ex_dot_pair1<6>(u0, u1, s_q, gl, D / 16, sa, sb);
            else ex_dot_pair1<(EX ? EX : 2)>(u0, u1, s_q, gl, D / 16, sa, sb);
        }
        if constexpr (V == kVarAvx512) {
            sa = group16_reduce(sa);
            sb = group16_reduce(sb);
        }
        if (gl == 0) {
            q_d[e0] = refined_distance(qc.scale, q_ip[e0], sa, qc.kbx, fa0, q_gadd[e0], fr0);
            if (has1) q_d[e1] = refined_distance(qc.scale, q_ip[e1], sb, qc.kbx, fa1, q_gadd[e1], fr1);
        }
    };

    struct Meta { float f_add, f_rescale, f_error, g_add, g_err, dotqc; };
    auto load_meta = [&](const WorkItem& w) -> Meta {
        const float* fac = reinterpret_cast<const float*>(P.blocks + (size_t)w.gblock * stride + (size_t)Dc * 4);
        const ProbeInfo pi = probe[w.rank_nvalid >> 6];
        Meta m;
        m.f_add = fac[l32]; m.f_rescale = fac[32 + l32]; m.f_error = fac[64 + l32];
        m.g_add = pi.g_add; m.g_err = pi.g_err; m.dotqc = pi.dotqc;
        return m;
    };
    // lower bound of one candidate as a function of its accumulator value: the exact operation sequence of
    // the epilogue (compute_batch_distances_u16, AVX2 body: only the first op is fused; kVarPortable: the scalar body, not
    // fused at all), so floating-point monotonicity carries over to the bound below
    auto lb_of = [&](const Meta& m, float accu_f, float& ip, float& est) -> float {
        ip = epi_ip(qc.delta, accu_f, qc.sum_vl, V == kVarPortable);
        const float tt = ip + qc.k1x;
        const float rs = m.f_rescale * tt;
        est = m.f_add + m.g_add;
        est = est + rs;
        const float er = m.f_error * m.g_err;
        return est - er;
    };
    // Block-level bound: accu of any code lies in [amin, amax] and lb is monotone in accu (direction = sign
    // of f_rescale), so min(lb(amin), lb(amax)) <= lb(true accu).  If that already reaches the (stale, hence
    // larger) threshold for every lane, the reference skips all of these candidates too and the block's
    // codes are never read.  Disabled when accu could wrap (amax > 65535) and when filtered diagnostics need
    // per-candidate filter tests.
    const bool bound_ok = qc.amax <= 65535.0f && !(P.filter && P.diag) && !P.no_block_bound;
    auto lane_prunable = [&](const WorkItem& w, const Meta& m, float T) -> bool {
        float d0, d1;
        const float a = lb_of(m, qc.amin, d0, d1), b = lb_of(m, qc.amax, d0, d1);
        const bool prunable = finite_f(a) && finite_f(b) && fminf(a, b) >= T;
        return (l32 >= (w.rank_nvalid & 63u)) || prunable;
    };

    // Uniform loop state (identical in every wave; advanced only from LDS values published before a barrier)
    uint32_t pos = 0;                 // next unexamined stream block
    uint32_t qhead = 0, qcount = 0;   // live-block FIFO
    uint32_t tile = 0;                // tiles published so far (buffer = tile & 1)
    // Blocks examined by the next fill step.  The first steps are small: with the threshold still at +inf the
    // block bound passes everything, and whatever is queued then is paid for at tile time (factor rows, a
    // barrier, usually no survivor).  Once the nearest lists have set a threshold the windows grow
    // (x kWinGrow per step, up to kFillK entries per scanner lane).
    uint32_t win = (uint32_t)kTB; // the first step: one tile's worth
    // replay-wave state
    const bool reg_heap = top_k < 64u * TR;                     // exact BinaryHeap emulation in registers (else in LDS)
    // RankRun from top_k = 64; below, the one-register sorted run (RankRun there costs the hot kernel 20 bytes of scratch at
    // five waves per SIMD, and at top_k = 10 most candidates are rejected by one scalar compare anyway)
    constexpr bool kRank = TR > 1;
    RegHeap<TR> rh; // the replay wave's top-k registers: exact heap, or (same registers) the bag
    rh.hd = 0; rh.hs = 0u; rh.xd = 0; rh.xs = 0u; rh.len = 0u;
    if (kRank && fast) RankRun<TR>::clear(rh); // keys, empty lanes marked
    int bag_dk = 0x7f800000; // RankRun: bits of the k-th distance (valid once the run holds top_k entries)
    bool tie_pending = false; // replay wave: a distance tie was met, the query will be re-run with the exact heap
    // LAZY TIES (the rule and its proof are at `amb_min` in scanw.hpp): equal distances do not end the fast pass; the smallest key
    // with which an element left (or was turned away) while its twin stayed is recorded, and the final run decides at the end of
    // the stream whether the reference's result depends on the layout of its heap.
    int amb_min = 0x7fffffff;
    // TIE LOG: every candidate a refine batch takes (a superset, in stream order, of the ones the reference evaluates) is written to
    // the query's log with its lower bound, refined distance and slot.  The reference's own loop over exactly these candidates —
    // `lower_bound >= distk` -> skip, push, pop — is a function of that sequence alone (a candidate outside the log has
    // lb >= a threshold that was already >= the reference's: skipped there too), so a tied query replays the log through the exact
    // heap instead of scanning its lists again.
    uint32_t log_n = 0; // replay wave, uniform: entries logged so far (may pass the capacity: then the log is not used)
    LdsHeap lh{heap_d, heap_s, 0};
#ifdef RBQ_STAMPS
    unsigned long long st_total = __builtin_amdgcn_s_memtime(), st_heavy = 0, st_waitA = 0, st_look = 0, st_fill = 0, st_a, st_b, st_c;
    uint32_t st_nheavy = 0, st_surv = 0, st_ntile = 0, st_dead = 0;
    uint32_t st_rounds = 0;
#define STAMP(x) x = __builtin_amdgcn_s_memtime()
    unsigned long long rp_collect = 0, rp_ref0 = 0, rp_replay = 0, rp_waitC = 0, rp_light = 0, rp_waitA = 0, r0 = 0, r1 = 0, rp_x1 = 0, rp_x2 = 0;
    unsigned long long mst[4] = {0, 0, 0, 0}; // RankRun::merge_batch phases (RBQ_STAMPS == 4)
#define RSTAMP(acc) do { r1 = __builtin_amdgcn_s_memtime(); acc += r1 - r0; r0 = r1; } while (0)
#else
#define STAMP(x)
#define RSTAMP(acc)
#endif

#ifdef RBQ_STAMPS
    const unsigned long long st_loop0 = __builtin_amdgcn_s_memtime();
    unsigned long long st_tiles = 0, st_t0 = 0;
#endif
  for (;;) { // a second pass only after a tie on the sorted fast path
    while (true) {
        if (pos < ns && qcount < (uint32_t)kTB) {
            // ---------------------------------------------------------------- fill step: examine `win` stream entries
            STAMP(st_c);
            if (scanner) {
                // kFillK stream entries per lane (entry k*192 + lane slot of the window): precomputed block-level
                // bound vs the threshold; compaction in stream order = (k, wave, lane) order
                const float T = s_T;
                const uint32_t wslot = wave * 64u + lane;
                WorkItem w[kFillK];
                bool live[kFillK];
                StreamItem si[kFillK];
#pragma unroll
                for (int k = 0; k < kFillK; ++k) {
                    const uint32_t wk = (uint32_t)k * (kNScan * 64u) + wslot;
                    si[k].gblock = 0; si[k].rank_nvalid = 0; si[k].lbmin = 0.0f; si[k].pad = 0;
                    live[k] = wk < win && pos + wk < ns;
                    if (live[k]) si[k] = wl[pos + wk];
                }
                unsigned long long lm[kFillK];
#pragma unroll
                for (int k = 0; k < kFillK; ++k) {
                    w[k].gblock = si[k].gblock; w[k].rank_nvalid = si[k].rank_nvalid;
                    if (live[k] && bound_ok && si[k].lbmin >= T) { // block_lbmin(): no real vector of the block can pass
                        live[k] = false;
                        if (count_skips) n_skip += w[k].rank_nvalid & 63u;
                    }
                    lm[k] = __ballot(live[k]);
                    if (lane == 0) s_fmask[k * kNScan + wave] = lm[k];
                }
                lds_barrier(); // X1: live masks published
                uint32_t total = 0;
#pragma unroll
                for (int j = 0; j < kNScan * kFillK; ++j) total += __popcll(s_fmask[j]);
                {
                    uint32_t base = 0; // running count of the sub-windows before k
#pragma unroll
                    for (int k = 0; k < kFillK; ++k) {
                        uint32_t cnt_k = 0;
#pragma unroll
                        for (int j = 0; j < kNScan; ++j) cnt_k += __popcll(s_fmask[k * kNScan + j]);
                        uint32_t offk = 0;
#pragma unroll
                        for (int j = 0; j < kNScan; ++j) if ((uint32_t)j < wave) offk += __popcll(s_fmask[k * kNScan + j]);
                        if (live[k]) s_queue[(qhead + qcount + base + offk + __popcll(lm[k] & ((1ull << lane) - 1ull))) % kQueueCap] = w[k];
                        base += cnt_k;
                    }
                }
                lds_barrier(); // X2: queue entries visible
                qcount += total;
            } else {
                lds_barrier(); // X1
                uint32_t total = 0;
#pragma unroll
                for (int j = 0; j < kNScan * kFillK; ++j) total += __popcll(s_fmask[j]);
                lds_barrier(); // X2
                qcount += total;
            }
            pos += win;
            win = win * kWinGrow < (uint32_t)kWindow ? win * kWinGrow : (uint32_t)kWindow;
#ifdef RBQ_STAMPS
            STAMP(st_b); st_fill += st_b - st_c;
#endif
            continue;
        }
        if (qcount == 0) break;
        // -------------------------------------------------------------------- tile step
        STAMP(st_t0);
        const uint32_t n = qcount < (uint32_t)kTB ? qcount : (uint32_t)kTB;
        const uint32_t buf = tile & 1u;
        if (scanner) {
          if constexpr (NB == 1) { // one block per half-wave and tile
            WorkItem wi_c;
            wi_c.gblock = 0; wi_c.rank_nvalid = 0;
            if (hw < n) wi_c = s_queue[(qhead + hw) % kQueueCap];
            const uint8_t* blk = P.blocks + (size_t)wi_c.gblock * stride;
            // The codes are requested together with the factor rows, not after the bound below: a queued block
            // already passed the block-level bound of the fill step, so it is almost always still alive, and the
            // two memory round trips overlap (the runtime-dimension path keeps the lazy order).
            CodeRegs<DT> cc;
            if (DT && hw < n) load_codes<DT>(cc, blk, l32);
            if (hw < n) { ++p_meta; if (DT) ++p_code; }
            const Meta m_c = load_meta(wi_c);
            const float T = s_T;
            // per-lane bound with the fresh threshold: the whole wave may be prunable without looking anything up
            const bool live_c = !bound_ok || (__ballot(lane_prunable(wi_c, m_c, T)) != ~0ull);
            const uint32_t nvalid = wi_c.rank_nvalid & 63u;
            const uint32_t slot = wi_c.gblock * 32u + l32;
            bool valid = l32 < nvalid;
            if (valid && P.filter) {
                const uint32_t id32 = (uint32_t)P.ids[slot];
                valid = ((uint64_t)id32 < P.filter_nbits) && ((P.filter[id32 >> 5] >> (id32 & 31u)) & 1u);
            }
            bool surv = false;
            float lb = 0.0f, ip = 0.0f, est = 0.0f;
#ifdef RBQ_STAMPS
            ++st_ntile; if (!live_c) ++st_dead;
#endif
            if (live_c) { // wave-uniform
                STAMP(st_a);
                if (!DT && hw < n) ++p_code;
                const uint32_t accu = (DT ? lookup_codes<DT>(cc, blk, l32, lut0) : accumulate_block_rt(blk, lut0, l32, Dc)) & 0xffffu;
#ifdef RBQ_STAMPS
                asm volatile("" :: "v"(accu));
                STAMP(st_b); st_look += st_b - st_a;
#endif
                lb = lb_of(m_c, (float)accu, ip, est);
                if (P.mstg) {
                    if (!finite_f(est)) valid = false;          // `if distance.is_finite()`
                    if (P.metric == 0) est = fmaxf(est, 0.0f);  // distance.max(0.0)
                    lb = est;                                   // f_error row and g_error are zero
                } else if (!finite_f(lb)) {
                    lb = P.metric == 0 ? 0.0f : -(m_c.dotqc + qc.qnorm);
                    // the reference skips iff `lower_bound >= distk` (src/ivf.rs:2054): a NaN bound (NaN query, inner product)
                    // is never skipped.  -inf decides every such test the same way and keeps `lb < T` usable below.
                    if (lb != lb) lb = -INFINITY;
                }
                surv = valid && (lb < T);
            }
            if (valid && !surv) ++n_skip;
            const unsigned long long bal = __ballot(surv);
            const uint32_t mask32 = (uint32_t)(bal >> (half * 32));
            if (l32 == 0) s_mask[buf * kTileBlocks + hw] = mask32;
            if (surv) {
                const uint32_t e = buf * kTileCand + hw * 32u + l32;
                q_slot[e] = slot;
                q_lb[e] = lb;
                q_ip[e] = ip;
                q_gadd[e] = m_c.g_add;
                q_d[e] = est;
            }
          } else {
            // half-wave hw scans blocks hw, hw + kTileBlocks, ... of the tile (NB of them); everything of all of them is requested
            // before the first lookup
            WorkItem wi_c[NB];
            const uint8_t* blk[NB];
            CodeRegs<DT> cc[NB];
            Meta m_c[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const uint32_t bi = hw + (uint32_t)(kTileBlocks * i);
                wi_c[i].gblock = 0; wi_c[i].rank_nvalid = 0;
                if (bi < n) wi_c[i] = s_queue[(qhead + bi) % kQueueCap];
                blk[i] = P.blocks + (size_t)wi_c[i].gblock * stride;
                // The codes are requested together with the factor rows, not after the bound below: a queued block
                // already passed the block-level bound of the fill step, so it is almost always still alive, and the
                // two memory round trips overlap (the runtime-dimension path keeps the lazy order).
                if (DT && bi < n) load_codes<DT>(cc[i], blk[i], l32);
                if (bi < n) { ++p_meta; if (DT) ++p_code; }
                m_c[i] = load_meta(wi_c[i]);
            }
            const float T = s_T;
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const uint32_t bi = hw + (uint32_t)(kTileBlocks * i);
                // per-lane bound with the fresh threshold: the whole wave may be prunable without looking anything up
                const bool live_c = !bound_ok || (__ballot(lane_prunable(wi_c[i], m_c[i], T)) != ~0ull);
                const uint32_t nvalid = wi_c[i].rank_nvalid & 63u;
                const uint32_t slot = wi_c[i].gblock * 32u + l32;
                bool valid = l32 < nvalid;
                if (valid && P.filter) {
                    const uint32_t id32 = (uint32_t)P.ids[slot];
                    valid = ((uint64_t)id32 < P.filter_nbits) && ((P.filter[id32 >> 5] >> (id32 & 31u)) & 1u);
                }
                bool surv = false;
                float lb = 0.0f, ip = 0.0f, est = 0.0f;
#ifdef RBQ_STAMPS
                ++st_ntile; if (!live_c) ++st_dead;
#endif
                if (live_c) { // wave-uniform
                    STAMP(st_a);
                    if (!DT && bi < n) ++p_code;
                    const uint32_t accu = (DT ? lookup_codes<DT>(cc[i], blk[i], l32, lut0) : accumulate_block_rt(blk[i], lut0, l32, Dc)) & 0xffffu;
#ifdef RBQ_STAMPS
                    asm volatile("" :: "v"(accu));
                    STAMP(st_b); st_look += st_b - st_a;
#endif
                    lb = lb_of(m_c[i], (float)accu, ip, est);
                    if (P.mstg) {
                        if (!finite_f(est)) valid = false;          // `if distance.is_finite()`
                        if (P.metric == 0) est = fmaxf(est, 0.0f);  // distance.max(0.0)
                        lb = est;                                   // f_error row and g_error are zero
                    } else if (!finite_f(lb)) {
                        lb = P.metric == 0 ? 0.0f : -(m_c[i].dotqc + qc.qnorm);
                        if (lb != lb) lb = -INFINITY; // (NaN is never `>= distk`: see the one-block form above)
                    }
                    surv = valid && (lb < T);
                }
                if (valid && !surv) ++n_skip;
                const unsigned long long bal = __ballot(surv);
                const uint32_t mask32 = (uint32_t)(bal >> (half * 32));
                if (l32 == 0) s_mask[buf * kTB + bi] = mask32;
                if (surv) {
                    const uint32_t e = buf * kTC + bi * 32u + l32;
                    q_slot[e] = slot;
                    q_lb[e] = lb;
                    q_ip[e] = ip;
                    q_gadd[e] = m_c[i].g_add;
                    q_d[e] = est;
                }
            }
          }
            STAMP(st_a);
            lds_barrier(); // A: this tile is published to the replay wave
#ifdef RBQ_STAMPS
            STAMP(st_b); st_waitA += st_b - st_a;
#endif
            if (fast && s_restart) break; // a tie was met: leave the pass now (every wave reads the flag behind the same barrier)
            uint32_t S = 0;
#pragma unroll
            for (int j = 0; j < kTB; ++j) S += __popc(s_mask[buf * kTB + j]);
#ifdef RBQ_STAMPS
            st_surv += S;
#endif
            if (S > kLightMax) { // synchronous tile: help refining round by round, then use the fresh threshold
                STAMP(st_a);
                while (true) {
                    lds_barrier(); // B_r: this round's refine batch (or the end marker) is published
                    const uint32_t nb = s_nbatch;
                    if (nb == kBatchDone) break;
#ifdef RBQ_STAMPS
                    ++st_rounds;
#endif
                    if (kDual) refine_pair(buf, nb & 0xffffu, tid >> 4, nb >> 16);
                    else refine_batch(buf, nb & 0xffffu, tid >> 4);
                    lds_barrier(); // C_r: refined distances visible to the replay wave
                }
#ifdef RBQ_STAMPS
                STAMP(st_b); st_heavy += st_b - st_a; ++st_nheavy;
#endif
            }
        } else {
            // ---------------------------------------------------------------- replay wave (uniform control flow)
            STAMP(r0);
            if (tie_pending && !tlog && lane == 0) s_restart = 1u; // (with a tie log the pass runs to its end: the log must be complete)
            lds_barrier(); // A
            RSTAMP(rp_waitA);
            if (fast && s_restart) break;
            // compaction in stream order: block by block, lane order within the block
            for (uint32_t b = half; b < (uint32_t)kTB; b += 2) {
                uint32_t base = 0;
                for (uint32_t j = 0; j < b; ++j) base += __popc(s_mask[buf * kTB + j]);
                const uint32_t m = s_mask[buf * kTB + b];
                if ((m >> l32) & 1u) s_list[base + __popc(m & ((1u << l32) - 1u))] = b * 32u + l32;
            }
            uint32_t S = 0;
#pragma unroll
            for (int j = 0; j < kTB; ++j) S += __popc(s_mask[buf * kTB + j]);
            S = __builtin_amdgcn_readfirstlane(S);
            const bool heavy = S > kLightMax;
            // Exact sequential replay of the reference's prune/push/pop loop in stream order, with LAZY refine:
            // a round takes the next survivors whose lb is below the CURRENT true threshold (a superset of the
            // ones the reference evaluates, since the threshold only shrinks), refines them in parallel and then
            // replays the examined stretch against the running threshold.
            uint32_t n_ref_tile = 0; // candidates taken for refinement in this tile (traffic counter)
            struct Batch { uint32_t p, np, ncol, e, logb; unsigned long long mt; int v_lb; };
            auto cur_distk = [&]() -> float {
                if (fast) return rh.len < top_k ? INFINITY : __int_as_float(!kRank ? SortedRun<TR>::kth(rh.hd, rh.xd, rh.len, top_k) : bag_dk);
                return reg_heap ? (rh.len < top_k ? INFINITY : __int_as_float(rh.d_at(0)))
                                : (lh.len < top_k ? INFINITY : heap_d[0]);
            };
            // next batch from position p: stretches without a wanted survivor are skipped (and counted) on the way;
            // the (at most G) wanted ones of the first stretch that has any go to s_batch
            auto collect = [&](uint32_t p, uint32_t G, float distk0) -> Batch {
                Batch bt;
                while (true) {
                    const uint32_t i = p + lane;
                    uint32_t e = 0;
                    float lbv = INFINITY;
                    if (i < S) { e = buf * kTC + s_list[i]; lbv = q_lb[e]; }
                    const bool want = i < S && lbv < distk0;
                    const unsigned long long m = __ballot(want);
                    uint32_t np = p + 64u < S ? p + 64u : S;
                    if (m == 0ull && np < S) { n_skip += np - p; p = np; continue; }
                    const uint32_t rank = __popcll(m & ((1ull << lane) - 1ull));
                    const bool take = want && rank < G;
                    const unsigned long long mt = __ballot(take);
                    if ((uint32_t)__popcll(m) > G) np = p + (63u - (uint32_t)__builtin_clzll(mt)) + 1u; // stop after the G-th taken
                    if (ex_bits && take) s_batch[rank] = s_list[i];
                    n_ref_tile += (uint32_t)__popcll(mt);
                    bt.p = p; bt.np = np; bt.ncol = (uint32_t)__popcll(mt); bt.e = e; bt.mt = mt; bt.v_lb = __float_as_int(lbv);
                    bt.logb = log_n;
                    if (tlog && fast) log_n += bt.ncol; // batches are collected in stream order (the replay may lag one batch behind)
                    return bt;
                }
            };
            // replay [bt.p, bt.np): only the taken survivors can pass the running threshold (it never grows, so
            // lb >= distk0 stays pruned); the rest of the stretch is counted as skipped in one step
            auto replay = [&](const Batch& bt) {
                int v_d = 0;
                uint32_t v_s = 0;
                if ((bt.mt >> lane) & 1ull) { v_d = __float_as_int(q_d[bt.e]); v_s = q_slot[bt.e]; }
                n_skip += (bt.np - bt.p) - bt.ncol;
                if (tlog && fast) { // tie log: the batch's candidates, in stream order (one 12-byte store per taken lane)
                    const uint32_t at = bt.logb + (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(bt.mt >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bt.mt, 0u));
                    if (((bt.mt >> lane) & 1ull) && at < P.tie_log_cap) {
                        uint32_t* ent = tlog + at * 3u; // (three dword stores from one address: no register triple to find)
                        ent[0] = (uint32_t)bt.v_lb; ent[1] = (uint32_t)v_d; ent[2] = v_s;
                    }
                }
#if RBQ_STAMPS == 4
                asm volatile("s_waitcnt lgkmcnt(0)" :: "v"(v_d), "v"(v_s) : "memory");
                RSTAMP(rp_x1); // the batch's distances have arrived from LDS
#endif
                if (fast && kRank) {
                    // the whole batch in one data-parallel step (RankRun)
#ifdef RBQ_STAMPS
                    const bool serial_counts = false; // (the diag slots carry cycle stamps in this build)
#else
                    const bool serial_counts = count_skips;
#endif
                    // (a tie is published before the next barrier A (or F), so that every wave reads the same flag after it)
                    tie_pending |= RankRun<TR>::replay(rh, top_k, bt.mt, bt.v_lb, v_d, v_s, lane, serial_counts,
                                                       reinterpret_cast<int*>(heap_d), heap_s, n_skip, n_ext, n_est, bag_dk, amb_min
#if RBQ_STAMPS == 4
                                                       , mst
#endif
                                                       );
#if RBQ_STAMPS == 4
                    RSTAMP(rp_x2); // the merge
#endif
                } else if (fast) replay_sorted(rh, top_k, bt.mt, bt.v_lb, v_d, v_s, lane, count_skips, n_skip, n_ext, n_est, amb_min);
                else if (reg_heap) replay_heap(rh, top_k, bt.mt, bt.v_lb, v_d, v_s, n_skip, n_ext, n_est);
                else {
                    for (unsigned long long todo = bt.mt; todo; todo &= todo - 1ull) { // uniform values, heap in LDS (top_k >= 64)
                        const uint32_t j = (uint32_t)__builtin_ctzll(todo);
                        const float lb = __int_as_float(__builtin_amdgcn_readlane(bt.v_lb, (int)j));
                        const float distk = lh.len < top_k ? INFINITY : heap_d[0];
                        if (lb >= distk) { ++n_skip; continue; }
                        ++n_ext;
                        const float d = __int_as_float(__builtin_amdgcn_readlane(v_d, (int)j));
                        if (!finite_f(d)) continue;
                        ++n_est;
                        if (lane == 0) {
                            lh.push(d, (uint32_t)__builtin_amdgcn_readlane((int)v_s, (int)j));
                            if (lh.len > top_k) lh.pop();
                        }
                        lh.len = (uint32_t)__builtin_amdgcn_readfirstlane((int)lh.len);
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        if (P.heap_ws) __threadfence_block(); // (global heap: lane 0's stores before the wave reads the root again)
                    }
                }
            };
            if (!(heavy && ex_bits)) {
                // light tile (or no ex codes): the wave refines with its own 4 groups while the scanners go on
                const uint32_t G = ex_bits ? (kDual ? 8u : 4u) : 64u;
                uint32_t p = 0;
                while (p < S) {
                    const Batch bt = collect(p, G, cur_distk());
                    if (ex_bits && bt.ncol) {
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        if (kDual) refine_pair(buf, bt.ncol, lane >> 4, 4u);
                        else refine_batch(buf, bt.ncol, lane >> 4);
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    }
                    replay(bt);
                    p = bt.np;
                }
                RSTAMP(rp_light);
            } else {
                // heavy tile, software-pipelined: round 0 is refined by all 16 groups; from then on the scanners'
                // 12 groups refine batch r+1 — collected with the threshold as it stands BEFORE batch r is
                // replayed, i.e. a superset again — while this wave replays batch r.
                STAMP(r0);
                constexpr uint32_t kPer = kDual ? 2u : 1u; // survivors per 16-lane group and round
                Batch cur = collect(0, kPer * (uint32_t)(kScanThreads / 16), cur_distk());
                RSTAMP(rp_collect);
                if (lane == 0) s_nbatch = cur.ncol | ((uint32_t)(kScanThreads / 16) << 16); // batch size | groups
                lds_barrier(); // B_0
                if (kDual) refine_pair(buf, cur.ncol, tid >> 4, (uint32_t)(kScanThreads / 16));
                else refine_batch(buf, cur.ncol, tid >> 4);
                lds_barrier(); // C_0
                RSTAMP(rp_ref0);
                while (cur.np < S) {
                    const Batch nxt = collect(cur.np, kPer * (uint32_t)(kNScan * 4), cur_distk());
                    if (lane == 0) s_nbatch = nxt.ncol | ((uint32_t)(kNScan * 4) << 16);
                    lds_barrier(); // B_r: the scanners start on batch r+1
                    RSTAMP(rp_collect);
                    replay(cur);
                    RSTAMP(rp_replay);
                    lds_barrier(); // C_r
                    RSTAMP(rp_waitC);
                    cur = nxt;
                }
                replay(cur);
                RSTAMP(rp_replay);
            }
            {
                const float tnew = cur_distk();
                if (lane == 0) {
                    s_T = tnew;
                    if (ex_bits && P.prof) s_misc[7] += n_ref_tile;
                }
            }
            if (heavy) {
                if (lane == 0) s_nbatch = kBatchDone;
                lds_barrier(); // final B: helpers leave the tile, fresh T is visible
            }
        }
#ifdef RBQ_STAMPS
        STAMP(st_b); st_tiles += st_b - st_t0;
#endif
        qhead = (qhead + n) % kQueueCap;
        qcount -= n;
        ++tile;
    }
    if (!scanner && fast && !tie_pending) tie_pending = lazy_tie_final(rh, kRank, top_k, amb_min, lane);
    if (!scanner && fast && tie_pending && tlog && log_n <= P.tie_log_cap) {
        // the tied query: the reference's loop over the logged candidates with the BinaryHeap emulation (this wave alone; the
        // scanners wait at barrier F).  The heap ends up where the re-scan would have left it.  (Not inlined: the cold path must not
        // take part in the register allocation of the scan loop — it cost the top_k = 100 instantiation a spill inside every tile.)
        __threadfence_block(); // (the log was written by this wave: its stores are complete before the loads below)
        if (lane == 0 && P.heap_restarts) atomicAdd(P.heap_restarts, 1u);
        rh = tie_log_replay<TR>(heap_d, heap_s, tlog, log_n, top_k, reg_heap, lane, P.tie_stats);
        lh.len = rh.len;
        fast = false; // (this wave only: the result is read from the heap below)
        tie_pending = false;
    }
    if (tie_pending && lane == 0) { s_restart = 1u; if (tlog && P.tie_stats) atomicAdd(P.tie_stats + 3, 1u); } // (lazy ties: decided by the final run)
    lds_barrier(); // F: the replay wave has consumed the last tile
    if (!s_restart) break;
    __syncthreads(); // every wave has seen the flag
    if (tid == 0) {
        s_T = INFINITY; s_restart = 0;
        if (P.heap_restarts) atomicAdd(P.heap_restarts, 1u);
    }
    fast = false;
    pos = 0; qhead = 0; qcount = 0; tile = 0; win = (uint32_t)kTB;
    ++p_pass;
    n_skip = 0; n_ext = 0; n_est = 0;
    rh.len = 0;
    bag_dk = 0x7f800000;
    tie_pending = false;
    amb_min = 0x7fffffff;
    __syncthreads();
  }
    if (!scanner) {
        if (fast) { // the sorted run: already ascending (TR > 1: keys)
#pragma unroll
            for (int r = 0; r < TR; ++r) {
                const uint32_t i = (uint32_t)r * 64u + lane;
                if (i < rh.len) {
                    heap_d[i] = __int_as_float(run_distance_bits(rh, r, kRank));
                    heap_s[i] = r == 0 ? rh.hs : rh.xs[r];
                }
            }
            if (lane == 0) s_len = rh.len;
        } else {
        // the exact heap: the register heap goes to LDS (the heap of top_k = 64 TR is there, or in the global workspace), final heap-sort
        if (reg_heap) lh.len = rh.len;
        spill_heap_sorted(rh, reg_heap, lh.len, heap_d, heap_s, lane, [] { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); });
        if (lane == 0) s_len = lh.len;
        if (P.heap_ws) __threadfence_block(); // (global heap: visible to the other waves behind the barrier below)
        }
        if (lane != 0) { n_skip = 0; n_ext = 0; n_est = 0; } // uniform counters: report them once
    }

    if (P.diag && n_skip) atomicAdd(s_nskip, n_skip);
    if (P.prof && scanner && l32 == 0 && p_meta) { atomicAdd(&s_misc[5], p_code); atomicAdd(&s_misc[6], p_meta); }
    __syncthreads();
    if (P.prof) {
        if (tid == 0) {
            unsigned long long* pc = P.prof + prof_stripe(q);
            atomicAdd(pc + kProfCodeBlocks, (unsigned long long)s_misc[5]);
            atomicAdd(pc + kProfMetaBlocks, (unsigned long long)s_misc[6]);
            atomicAdd(pc + kProfStreamEntries, (unsigned long long)ns * p_pass);
            atomicAdd(pc + kProfQueries, 1ull);
        }
        if (wave == (uint32_t)kNScan && lane == 0 && ex_bits) atomicAdd(P.prof + prof_stripe(q) + kProfExEvals, (unsigned long long)s_misc[7]);
    }
    const uint32_t len = s_len;
    for (uint32_t i = tid; i < top_k; i += kScanThreads) {
        uint64_t id = ~0ull;
        float sc = __int_as_float(0x7fc00000);
        if (i < len) {
            id = P.ids[heap_s[i]];
            sc = (P.metric == 0 || P.mstg) ? heap_d[i] : -heap_d[i]; // MSTG reports the distance for both metrics
        }
        P.out_ids[(size_t)q * top_k + i] = id;
        P.out_scores[(size_t)q * top_k + i] = sc;
    }
#ifdef RBQ_STAMPS
#if RBQ_STAMPS == 3
    if (tid == 0 && P.diag) { // scanner wave 0: lookup time, wait at barrier A, live tiles
        P.diag[(size_t)q * 3 + 0] = (st_look & 0xffffffffull) | (st_waitA << 32);
        P.diag[(size_t)q * 3 + 1] = (unsigned long long)(st_ntile - st_dead) | ((unsigned long long)st_surv << 32);
        P.diag[(size_t)q * 3 + 2] = (st_fill & 0xffffffffull) | ((unsigned long long)st_nheavy << 32);
    }
#endif
    if (RBQ_STAMPS == 1 && tid == 0 && P.diag) { // diagnostic build: the diag slots carry cycle stamps of scanner wave 0 instead
        const unsigned long long st_total0 = st_total;
        st_total = __builtin_amdgcn_s_memtime() - st_total;
        P.diag[(size_t)q * 3 + 0] = (st_heavy & 0xffffffffull) | ((unsigned long long)st_rounds << 32);
        P.diag[(size_t)q * 3 + 1] = (st_total & 0xffffffffull) | (((st_loop0 - st_total0) & 0xffffull) << 32) | ((unsigned long long)(tile & 0xffff) << 48);
        P.diag[(size_t)q * 3 + 2] = (unsigned long long)(st_tiles & 0xffffffffull) | (st_fill << 32);
    }
    if (wave == (uint32_t)kNScan && lane == 0) {
        P.out_counts[q] = len;
#if RBQ_STAMPS == 4
        if (P.diag) {
            P.diag[(size_t)q * 3 + 0] = (rp_x1 & 0xffffffffull) | (rp_x2 << 32);
            P.diag[(size_t)q * 3 + 1] = (mst[0] & 0xffffffffull) | (mst[1] << 32);
            P.diag[(size_t)q * 3 + 2] = (mst[2] & 0xffffffffull) | (rp_waitA << 32);
        }
#endif
#if RBQ_STAMPS == 2
        if (P.diag) {
            P.diag[(size_t)q * 3 + 0] = (rp_collect & 0xffffffffull) | (rp_ref0 << 32);
            P.diag[(size_t)q * 3 + 1] = (rp_replay & 0xffffffffull) | (rp_waitC << 32);
            P.diag[(size_t)q * 3 + 2] = (rp_light & 0xffffffffull) | (rp_waitA << 32);
        }
#endif
    }
#else
    if (wave == (uint32_t)kNScan && lane == 0) {
        P.out_counts[q] = len;
        if (P.diag) {
            P.diag[(size_t)q * 3 + 0] = n_est;
            // + the vectors of probed lists that the probe selection proved skipped as a whole (never streamed)
            P.diag[(size_t)q * 3 + 1] = *s_nskip + (P.dead_skipped ? P.dead_skipped[q] : 0u);
            P.diag[(size_t)q * 3 + 2] = ex_bits ? n_ext : 0;
        }
    }
#endif
}

} // namespace rbq
