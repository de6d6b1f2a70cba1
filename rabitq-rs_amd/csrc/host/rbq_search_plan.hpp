// rbq_search_plan.hpp — the routing of ONE device search call (api_search.hip: search_core -> search_front -> scan_stage): which
// preparation, ranking, selection and scan kernel a call of a given shape runs, on which tile, in how many split-K parts, and
// which workspace buffers it needs.  Every threshold is evaluated once, here; the HIP side only sizes buffers, fills the
// kernels' parameter blocks and launches what the plan says.  Pure C++ (no HIP): tests/plancheck_main.cpp builds it with
// -fsanitize=address,undefined and tests/test_search_plan_host.py checks the table on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "rbq_scan_limits.hpp"

namespace rbq_host {

using rbq::kLdsPerWorkgroupMax;
using rbq::kNprobeMax;
using rbq::kTopKMax;
using rbq::kTopKRegMax;

// scan_wave = 2: batches of at least this many queries go to k_scanw (a query costs one resident wave instead of four: the
// pipelined rate), smaller ones to k_scan (four waves shorten ONE query's chain: the latency of a small call)
constexpr uint64_t kScanWaveMinQueries = 128;
// Latency-first front (latency.hpp): one launch rotates the query, builds its LUT and scores EVERY list exactly, spread over
// n_lists / 32 workgroups per query.  It re-reads the centroid table once per query, so it serves calls of a few queries only
// (every query's pass over the table must stay a few microseconds: n_lists x D x 4 bytes x nq within kLatMaxBytes).
constexpr uint64_t kLatMaxQueries = 4; // (measured, GIST-1M shape: 1 / 2 / 4 queries per call -12 / -10 / -12 us against prep + GEMM; 8: no gain)
constexpr uint64_t kLatMaxBytes = 96ull << 20;
constexpr uint64_t kSplitKMaxCallQueries = 256; // calls up to here split the ranking GEMM's K loop over grid.z
constexpr uint64_t kPrepWgMaxQueries = 512; // up to here the preparation runs one WORKGROUP per query (latency.hpp without the scorers)
// ranking GEMM tiles: from this many 128 x 128 tiles the chip is full of them (big), from this many 256 x 128 tiles the 256-wide
// form pays (wide; cfg5: 16 384 queries x 65 536 lists)
constexpr uint64_t kBigMinTiles = 192, kWideMinTiles = 2048;

// What routing reads of a call and of the index it searches.
struct SearchShape {
    uint64_t nq = 0;          // queries of this launch chain
    uint64_t call_nq = 0;     // queries of the WHOLE host call it belongs to (0: a device-entry call — its own nq counts)
    uint32_t top_k = 0;       // (range: the capacity of a query's output row)
    uint32_t nprobe = 0;      // as requested; the plan clamps it to [1, n_lists]
    uint64_t n_lists = 0;
    uint32_t D = 0, Dc = 0;   // padded dimension; rounded up to 64
    int rotator = 0;          // RBQ_ROTATOR_*: 0 matrix, 1 FHT-Kac, 2 none
    uint32_t ex_bits = 0;
    bool rank_f16_ok = false; // the index holds a usable f16 image of its centroids
    bool has_filter = false, has_diag = false;
    bool range = false;         // range search: eager selection, k_range instead of the top-k scan
    bool latency_first = false; // the chain belongs to a host call that waits for it (Workspace::latency_first)
    bool mstg = false;          // the MSTG posting scan: its own front has run, only the scan is planned (nprobe: the list stride)
    bool probe_installed = false; // rbq_debug_stage_resources: nothing is launched
    // prefix sums of the per-list block counts sorted descending ([n_lists + 1]; null: wl_stride is not the plan's)
    const uint64_t* nblk_desc_prefix = nullptr;
    size_t nblk_desc_prefix_len = 0;
};

// The option fields that routing reads (api.hpp fills it from Options in one place: route_options()).
struct RouteOptions {
    bool exact_rank = false, f32_rank = false, wg_prep = false;
    int latency_path = 1, rank_ksplit = 1, rank_tile = 0, rank_f16 = -1;
    bool rank_planar = false;
    uint32_t stage_mask = 0xf;
    bool lazy_select = true, lazy_filter = true, head_exact = true, no_block_bound = false;
    int scan_wave = 2;
    bool tie_log = true;
    uint32_t tie_log_cap = 0;
    bool exact_heap = false;
};

enum class PrepForm : uint8_t {
    none,        // the MSTG scan (prepared by its own front)
    prep,        // k_prep: one workgroup per query (the matrix rotator, option wg_prep)
    prep_wave,   // k_prep_wave: one wave per query (full batches)
    wg,          // k_lat_front as preparation only: one workgroup per query, the ranking GEMM follows
    wg_zero,     // ... which also clears the score rows: a split-K GEMM adds its parts to them
    lat_scorers, // k_lat_front with its scorers: preparation AND the exact score of every list in one launch
};
enum class RankRoute : uint8_t {
    none,   // the latency front has scored every list (or: the MSTG scan)
    exact,  // k_rank_scores: exact all-pairs scores (option exact_rank, nprobe > kNprobeMax)
    f32,    // k_rank_mfma: f32 MFMA GEMM (option f32_rank, D % 64 != 0)
    bf16x3, // k_rank_bf16_db: split-bf16, three products
    f16,    // k_rank_f16_db: one f16 product
};

struct SearchPlan {
    uint32_t nprobe = 1;      // clamped to [1, n_lists]
    bool big_nprobe = false;  // nprobe > kNprobeMax: exact ranking and selection, the key window in global memory
    uint64_t wl_stride = 0;   // stream entries per query
    uint32_t stage_mask = 0xf; // (diagnostic option: bit s = stage s is launched)
    PrepForm prep = PrepForm::none;
    RankRoute rank = RankRoute::none;
    uint32_t tile = 64;       // ranking GEMM: 64, 128 or 256 (256: split routes only)
    uint32_t ksplit = 1;      // parts of the GEMM's K loop over grid.z
    bool planar = false;      // TEST ONLY: the split-bf16 GEMM reads planar copies of its operands, made per call
    bool exact_select = false; // k_select after exact scores (else k_select_mfma: shortlist + exact canonical scores)
    bool lazy = false;        // k_select_mfma drops lists that are provably skipped as a whole
    bool wave_kernel = false; // k_scanw requested (launch_scan falls back to k_scan where k_scanw does not serve the shape)
    bool heap_in_global = false; // the top-k heap does not fit the LDS: ScanParams::heap_ws
    bool tie_log = false;
    uint32_t tie_log_cap = 0; // entries per query
    // workspace buffers beyond the ones every call has
    bool need_rot_hl = false, need_rot_f16 = false, need_rank_resid = false, need_rank_planes = false, need_key_window = false;

    bool lat_front() const { return prep == PrepForm::lat_scorers; }
    bool split_route() const { return rank == RankRoute::bf16x3 || rank == RankRoute::f16; }
};

// The couplings between a plan's fields that the kernels rely on.
inline bool plan_search_ok(const SearchPlan& p, const SearchShape& s, const RouteOptions& o) {
    const bool split_k = p.ksplit > 1;
    return p.nprobe >= 1 && (s.n_lists == 0 || p.nprobe <= s.n_lists) &&
           // a split-K GEMM ADDS into score rows that only the zeroing preparation clears; its eps is derived for bf16x3 on <= 128 tiles
           (!split_k || (p.prep == PrepForm::wg_zero && p.rank == RankRoute::bf16x3 && p.tile <= 128 && p.ksplit <= 4)) &&
           (p.rank != RankRoute::f16 || (p.ksplit == 1 && !p.planar && !p.lat_front() && p.need_rot_f16 && p.need_rank_resid)) &&
           (p.lat_front() == (p.rank == RankRoute::none && !s.mstg)) &&
           (p.tile == 64 || p.tile == 128 || p.tile == 256) && (p.tile != 256 || p.split_route()) &&
           ((p.rank == RankRoute::exact) == p.exact_select) && (p.big_nprobe == p.need_key_window) && (!p.big_nprobe || p.exact_select) &&
           (!p.planar || (p.rank == RankRoute::bf16x3 && p.need_rank_planes)) &&
           (!p.lazy || (!s.range && !o.no_block_bound && !p.exact_select)) &&
           (!p.tie_log || (!p.wave_kernel && p.tie_log_cap > 0 && s.top_k <= kTopKRegMax)) &&
           (!s.range || (!p.wave_kernel && !p.tie_log && !p.heap_in_global));
}

inline SearchPlan plan_search(const SearchShape& s, const RouteOptions& o) {
    SearchPlan p;
    const uint32_t nlist = (uint32_t)s.n_lists, D = s.D;
    const uint64_t nq = s.nq;
    p.stage_mask = o.stage_mask;

    // ---- the scan (the only part an MSTG posting scan reads) ------------------------------------------------------------------
    if (!s.range) {
        // scan_wave = 2 (default): the wave-per-query kernel serves the pruned regime of batches large enough to fill the chip with
        // waves; with the block bound off (every probed block streamed: the roofline configuration) the four-wave kernel streams
        // at twice its rate and serves the call.  Results are identical either way.
        // A host call (rbq_search_batch) that waits for ONE chain of kernels is served by the kernel with the shorter chain (k_scan's
        // four waves finish a 1024-query launch in 0.10 ms, k_scanw's single wave in 0.14 ms) until the call is large enough for the rate
        // to matter more than the last chain's latency.
        p.wave_kernel = o.scan_wave == 1 || (o.scan_wave == 2 && nq >= kScanWaveMinQueries && !o.no_block_bound && !s.latency_first);
        // tie log (k_scan, no diagnostics, top-k in registers): a tied query replays its logged candidates instead of its lists
        if (o.tie_log && !p.wave_kernel && !s.has_diag && !s.mstg && s.top_k >= 1 && s.top_k <= kTopKRegMax && !o.exact_heap && !s.probe_installed) {
            // entries per query: ~80 candidates are refined per query at top_k = 10 and ~400 at top_k = 100 on the bench data; a query that
            // logs more than the capacity is scanned again, as before (option tie_log_cap: tests of that path)
            const uint32_t cap = o.tie_log_cap ? o.tie_log_cap : (s.top_k < 64u ? 2048u : 8192u);
            if (nq * cap * 12u <= (1ull << 30)) { p.tie_log = true; p.tie_log_cap = cap; }
        }
        // top_k > kTopKMax, or a heap that does not fit the LDS beside the rest: the heap in global memory — slow, but served (the
        // reference accepts any top_k).  MSTG search never evaluates the ex codes.
        p.heap_in_global = s.top_k > kTopKMax || rbq::scan_lds_bytes(s.Dc, D, s.mstg ? 0u : s.ex_bits, s.top_k) > kLdsPerWorkgroupMax;
    }
    if (s.mstg) { p.nprobe = s.nprobe; return p; }

    // ---- the probes ------------------------------------------------------------------------------------------------------------
    p.nprobe = std::min(std::max(s.nprobe, 1u), std::max(nlist, 1u));
    // nprobe > kNprobeMax: the exact all-pairs ranking with its key window in global memory (slow, but served: the reference clamps
    // nprobe to n_lists)
    p.big_nprobe = p.need_key_window = p.nprobe > kNprobeMax;
    if (s.nblk_desc_prefix && s.nblk_desc_prefix_len)
        p.wl_stride = std::max<uint64_t>(s.nblk_desc_prefix[std::min<size_t>(p.nprobe, s.nblk_desc_prefix_len - 1)], 1);
    p.exact_select = o.exact_rank || p.big_nprobe;

    // ---- the front -------------------------------------------------------------------------------------------------------------
    const bool split_rank = !o.exact_rank && !o.f32_rank && D % 64 == 0; // k_rank_bf16_db / k_rank_f16_db (else k_rank_mfma)
    const bool full_mask = o.stage_mask == 0xfu;
    // the latency kernel serves FHT-Kac and no rotator (the matrix rotator is O(D^2) per query: k_prep)
    const bool lat_kernel = o.latency_path && s.rotator != 0 && !o.wg_prep && D % 16 == 0;
    // small calls: prep + exact scores of every list in one launch (the ranking GEMM and its launch boundary are skipped)
    const bool lat_front = lat_kernel && nq <= kLatMaxQueries && !p.exact_select && !o.f32_rank && (uint64_t)nlist * D * 4 * nq <= kLatMaxBytes && full_mask;
    // batches a caller waits for (a few hundred queries: the chip is not full): a workgroup per query — the serial sums on one
    // wave while the others build the LUT (latency.hpp, preparation only); full batches keep one wave per query (k_prep_wave)
    const bool wg_form = lat_kernel && nq <= kPrepWgMaxQueries;

    // ONE tile decision.  Option rank_tile: 0 = by problem size, 64 / 128 / 256 = forced (tests; A/B)
    const uint64_t rows128 = (nq + 127) / 128;
    const bool big = o.rank_tile == 64 ? false : o.rank_tile == 128 ? true : (uint64_t)((nlist + 127) / 128) * rows128 >= kBigMinTiles;
    const bool wide_by_size = (uint64_t)((nlist + 255) / 256) * rows128 >= kWideMinTiles;
    // (the 256 form exists for the split GEMMs only: k_rank_mfma, and a call whose GEMM does not run, stay on the square tiles)
    const bool wide = split_rank && !p.exact_select && !lat_front && (o.rank_tile == 256 || (o.rank_tile == 0 && wide_by_size));
    p.tile = wide ? 256u : big ? 128u : 64u;

    // split-K of the ranking GEMM for batches whose tiles leave the chip idle (the rows are cleared by the workgroup-per-query preparation)
    // (only when the whole CALL is small: the sub-batches of a 1024-query host call overlap each other, and the extra workgroups and
    // atomics of a split GEMM then cost more than its shorter K loop saves — 277 -> 295 us per call, measured)
    uint32_t ksplit = 1;
    if (o.rank_ksplit && wg_form && !lat_front && (s.call_nq ? s.call_nq : nq) <= kSplitKMaxCallQueries && split_rank && !p.big_nprobe && full_mask) {
        const uint32_t T = big ? 128u : 64u; // (the 256 form has no split-K: see below)
        const uint64_t tiles = (uint64_t)((nlist + T - 1) / T) * ((nq + T - 1) / T);
        ksplit = tiles >= 512 ? 1u : (tiles >= 256 ? 2u : 4u);
        while (ksplit > 1 && (D / 32) / ksplit < 6) ksplit >>= 1; // (at least six slabs per part)
        // (option: forced; at most 4 parts, the most the eps of k_select_mfma is derived for — rank_mfma.hpp header)
        if (o.rank_ksplit > 1) ksplit = (uint32_t)std::min(o.rank_ksplit, 4);
    }
    p.prep = lat_front ? PrepForm::lat_scorers
             : wg_form ? (ksplit > 1 ? PrepForm::wg_zero : PrepForm::wg)
             : (s.rotator == 0 || o.wg_prep) ? PrepForm::prep : PrepForm::prep_wave;

    // one-product f16 ranking (rank_mfma.hpp header, "ONE f16 PRODUCT").  Possible: the index qualifies, the call ranks on the split GEMM
    // without split-K, planar copies or the exact front.  By rule (rank_f16 = -1): on top of that no forced tile, a big or wide call (the
    // GEMM is a stage worth routing) and D >= 256.
    const bool f16_possible = s.rank_f16_ok && split_rank && ksplit == 1 && !o.rank_planar && !p.big_nprobe && !lat_front;
    const bool f16 = o.rank_f16 != 0 && f16_possible && (o.rank_f16 > 0 || (o.rank_tile == 0 && (big || wide_by_size) && D >= 256));
    p.rank = p.exact_select ? RankRoute::exact : lat_front ? RankRoute::none : !split_rank ? RankRoute::f32 : f16 ? RankRoute::f16 : RankRoute::bf16x3;
    // The 256 grid has no z: on a call that asked for parts (a forced tile of 256 below the wide size, or forced parts on a wide
    // call) the GEMM runs unsplit.  As before the plan existed, the preparation has cleared the rows all the same and the f16 rule
    // above has seen the parts asked for.
    p.ksplit = wide ? 1u : ksplit;
    p.planar = o.rank_planar && p.rank == RankRoute::bf16x3 && !s.probe_installed;
    p.need_rot_hl = split_rank;
    p.need_rot_f16 = p.need_rank_resid = p.rank == RankRoute::f16;
    p.need_rank_planes = p.planar;

    // ---- the selection ---------------------------------------------------------------------------------------------------------
    // lazy selection: not with a filter (filtered vectors are never pushed, so no select-time bound of the k-th distance
    // exists) and not when every probed block is to be streamed
    // (round 4: under a filter the exact head evaluation can still bound the k-th distance — it looks at real vectors and counts
    // the ones that pass; with diagnostics the skip counter of a dropped list would need every id's filter bit: eager then)
    // `range`: the selection is eager (no threshold exists to drop a list against)
    const bool lazy_with_filter = o.lazy_filter && o.head_exact && !s.has_diag;
    p.lazy = !p.exact_select && o.lazy_select && (!s.has_filter || lazy_with_filter) && !o.no_block_bound && !s.range;
    return p;
}

} // namespace rbq_host
