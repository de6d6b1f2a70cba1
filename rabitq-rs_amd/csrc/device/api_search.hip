// api_search.hip — the IVF search: the device entry and the host entry (rbq_search_batch, one replica or N).  The hot path
// (search_host -> search_device -> search_front -> scan_stage, or range_stage while the option range_search is on) stays in this one
// unit; api_mstg_search.hip shares its workspaces and scan_stage.  Which kernels a call runs is decided once, in plain host code
// (rbq_host::plan_search, csrc/host/rbq_search_plan.hpp); this unit sizes buffers, fills parameter blocks and launches what the plan says.
#include "api.hpp"

using namespace rbq_api;

namespace rbq_api {
namespace {
// The WHOLE range [p, p + bytes) is page-locked host memory of one allocation / registration: the kernels write (and the
// DMA engines read) every byte of it, so a registration that covers only the first pages must not pass.
bool is_pinned_host_range(const void* p, size_t bytes) {
    if (!p) return false;
    hipPointerAttribute_t a, b;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (a.type != hipMemoryTypeHost) return false;
    if (bytes <= 1) return true;
    const uint8_t* last = (const uint8_t*)p + bytes - 1;
    if (hipPointerGetAttributes(&b, last) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (b.type != hipMemoryTypeHost) return false;
    // same mapping: the device-side addresses of the two ends are as far apart as the host-side ones
    if (a.devicePointer && b.devicePointer && (const uint8_t*)b.devicePointer - (const uint8_t*)a.devicePointer != (ptrdiff_t)(bytes - 1)) return false;
    if (a.hostPointer && b.hostPointer && (const uint8_t*)b.hostPointer - (const uint8_t*)a.hostPointer != (ptrdiff_t)(bytes - 1)) return false;
    return true;
}
} // namespace

// ---- shared with api_mstg_search.hip (declared in api.hpp) ---------------------------------------------------------------------
Workspace* take_ws(Replica* ix) {
    {
        std::lock_guard<std::mutex> g(ix->mu);
        if (!ix->pool.empty()) { Workspace* w = ix->pool.back(); ix->pool.pop_back(); return w; }
    }
    Workspace* w = new Workspace();
    if (hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess) { delete w; return nullptr; }
    if (hipEventCreateWithFlags(&w->done, hipEventDisableTiming) != hipSuccess) { (void)hipStreamDestroy(w->stream); delete w; return nullptr; }
    return w;
}
void give_ws(Replica* ix, Workspace* w) {
    std::lock_guard<std::mutex> g(ix->mu);
    ix->pool.push_back(w);
}

// One workspace per caller stream, never handed to anyone else: successive calls on the same stream are
// stream-ordered, so their kernels may share the scratch buffers without any host synchronisation.
Workspace* stream_workspace(Replica* ix, hipStream_t s) {
    std::lock_guard<std::mutex> lk(ix->mu);
    Workspace*& slot = ix->stream_ws[s];
    if (!slot) slot = new Workspace();
    return slot;
}

int check_query_args(const rbq_index* h, uint32_t query_dim) {
    if (!h || h->reps.empty()) return fail(RBQ_INVALID_CONFIG, "null index");
    const Replica* ix = h->reps[0];
    if (ix->n_vectors == 0) return fail(RBQ_EMPTY_INDEX, "index is empty");
    if (query_dim != ix->dim) {
        char b[96];
        std::snprintf(b, sizeof b, "expected %u, got %u", ix->dim, query_dim);
        return fail(RBQ_DIMENSION_MISMATCH, b);
    }
    return RBQ_OK;
}

int check_query_pointer(const rbq_index* h, const void* queries) {
    if (!query_rows(h->reps[0], 0).aligned(queries)) return fail(RBQ_INVALID_CONFIG, "queries: pointer not aligned to its 16-bit elements");
    return RBQ_OK;
}

Replica* replica_of_pointer(rbq_index* h, const void* dptr) {
    if (h->reps.size() == 1) return h->reps[0];
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, dptr) == hipSuccess) {
        for (Replica* r : h->reps) if (r->device == a.device) return r;
    } else {
        (void)hipGetLastError();
    }
    return h->reps[0];
}

rbq_host::SearchPlan search_plan(const Replica* ix, const Workspace* w, uint64_t nq, uint32_t top_k, uint32_t nprobe, bool has_filter,
                                 bool has_diag, bool range, bool mstg) {
    rbq_host::SearchShape s;
    s.nq = nq; s.call_nq = w->call_nq; s.top_k = top_k; s.nprobe = nprobe; s.n_lists = ix->n_lists; s.D = ix->D; s.Dc = ix->Dc;
    s.rotator = ix->rotator; s.ex_bits = ix->ex_bits; s.rank_f16_ok = ix->rank_f16_ok; s.has_filter = has_filter; s.has_diag = has_diag;
    s.range = range; s.latency_first = w->latency_first; s.mstg = mstg; s.probe_installed = stage_probes() != nullptr;
    if (!mstg) { s.nblk_desc_prefix = ix->nblk_desc_prefix.data(); s.nblk_desc_prefix_len = ix->nblk_desc_prefix.size(); }
    return rbq_host::plan_search(s, route_options(ix->opt));
}

// k_scan launch shared by the IVF search and the MSTG posting-list scan
int scan_stage(Replica* ix, Workspace* w, const rbq_host::SearchPlan& plan, uint64_t nq, uint32_t probe_stride, uint32_t top_k,
               uint64_t wl_stride, const uint32_t* d_filter, uint64_t filter_nbits, uint64_t* d_ids, float* d_scores, uint32_t* d_counts,
               rbq_diag* d_diag, bool mstg, const uint32_t* d_dead_skipped, hipStream_t stream, const uint64_t* d_slot_ids) {
    ProfScope ps(ix, 3, stream, /*ext=*/true);
    ScanParams P;
    // (d_slot_ids, the refined MSTG search: the identity slot map stands in for the ids, so the result names positions)
    P.blocks = (const uint8_t*)ix->blocks.p; P.ids = d_slot_ids ? d_slot_ids : (const uint64_t*)ix->ids.p; P.ex_codes = (const uint8_t*)ix->ex.p;
    P.f_add_ex = (const float*)ix->fadd_ex.p; P.f_rescale_ex = (const float*)ix->fres_ex.p;
    P.lut = (const uint8_t*)w->lut.p; P.rot = (const float*)w->rot.p; P.consts = (const QueryConsts*)w->consts.p;
    P.probe = (const ProbeInfo*)w->probe.p; P.wl = (const StreamItem*)w->wl.p; P.nstream = (const uint32_t*)w->nstream.p;
    P.filter = d_filter; P.filter_nbits = filter_nbits; P.wl_stride = wl_stride;
    P.out_ids = d_ids; P.out_scores = d_scores; P.out_counts = d_counts; P.diag = (unsigned long long*)d_diag;
    P.D = ix->D; P.Dc = ix->Dc; P.nprobe = probe_stride; P.top_k = top_k; P.metric = ix->metric;
    P.ex_bits = mstg ? 0u : ix->ex_bits; // MSTG search never evaluates the ex codes (src/mstg/index.rs:216-330)
    P.no_block_bound = ix->opt.no_block_bound ? 1u : 0u;
    P.exact_heap = ix->opt.exact_heap ? 1u : 0u;
    P.heap_restarts = (unsigned int*)ix->fallbacks.p + 1;
    P.tie_stats = (unsigned int*)ix->fallbacks.p + 4;
    P.mstg = mstg ? 1u : 0u;
    P.prof = (ix->profiling && ix->opt.profile_counters) ? (unsigned long long*)ix->prof.p : nullptr;
    P.dead_skipped = d_dead_skipped;
    P.numeric_variant = ix->opt.numeric_variant;
    P.wave_kernel = plan.wave_kernel ? 1u : 0u;
    P.tie_log = nullptr; P.tie_log_cap = 0;
    if (plan.tie_log) {
        if (w->tie_log.ensure((size_t)nq * plan.tie_log_cap * 12u) == RBQ_OK) { P.tie_log = (uint32_t*)w->tie_log.p; P.tie_log_cap = plan.tie_log_cap; }
        else { (void)hipGetLastError(); g_err.clear(); } // (no memory for the log: the call is served without it)
    }
    P.heap_ws = nullptr;
    if (plan.heap_in_global) {
        int rc = w->heap_ws.ensure((size_t)nq * 2 * ((size_t)top_k + 1) * 4);
        if (rc) return rc;
        P.heap_ws = (uint32_t*)w->heap_ws.p;
    }
    HIP_TRY(launch_scan(P, (uint32_t)nq, ix->device, stream, ps.start(), ps.stop()));
    return RBQ_OK;
}

// k_range launch: the range search's stage, where a top-k call has scan_stage.  `cap` = the capacity of a query's output row.  No heap
// workspace, no tie log and no dead_skipped: the range path selects eagerly, so every probed list is in the stream.
// While the option range_exact is on (search_device has checked that raw vectors are attached and the rerank is on) the exact
// variant is launched: the same parameters, plus the caller's queries, the raw rows and the exact radius x.
int range_stage(Replica* ix, Workspace* w, const float* d_queries, uint64_t nq, uint32_t probe_stride, uint32_t cap, uint64_t wl_stride,
                const uint32_t* d_filter, uint64_t filter_nbits, uint64_t* d_ids, float* d_scores, uint32_t* d_counts,
                rbq_diag* d_diag, hipStream_t stream) {
    ProfScope ps(ix, 3, stream, /*ext=*/true); // (the profile stage "scan" times k_range while the option is on)
    RangeExactParams P; // (the estimate-only launch takes its RangeParams part)
    P.blocks = (const uint8_t*)ix->blocks.p; P.ids = (const uint64_t*)ix->ids.p; P.ex_codes = (const uint8_t*)ix->ex.p;
    P.f_add_ex = (const float*)ix->fadd_ex.p; P.f_rescale_ex = (const float*)ix->fres_ex.p;
    P.lut = (const uint8_t*)w->lut.p; P.rot = (const float*)w->rot.p; P.consts = (const QueryConsts*)w->consts.p;
    P.probe = (const ProbeInfo*)w->probe.p; P.wl = (const StreamItem*)w->wl.p; P.nstream = (const uint32_t*)w->nstream.p;
    P.filter = d_filter; P.filter_nbits = filter_nbits; P.wl_stride = wl_stride;
    P.out_ids = d_ids; P.out_scores = d_scores; P.out_counts = d_counts; P.diag = (unsigned long long*)d_diag;
    P.D = ix->D; P.Dc = ix->Dc; P.nprobe = probe_stride; P.top_k = cap; P.metric = ix->metric; P.ex_bits = ix->ex_bits;
    P.no_block_bound = ix->opt.no_block_bound ? 1u : 0u;
    P.exact_heap = 0; P.heap_restarts = nullptr; P.tie_stats = nullptr; P.mstg = 0; P.prof = nullptr; P.heap_ws = nullptr;
    P.dead_skipped = nullptr; P.wave_kernel = 0; P.tie_log = nullptr; P.tie_log_cap = 0;
    P.numeric_variant = ix->opt.numeric_variant;
    // the caller's radius bounds the distance for L2 and the score for inner product: both are `distance < R` on the internal distance
    float r;
    std::memcpy(&r, &ix->opt.range_radius_bits, 4);
    P.R = ix->metric == 0 ? r : -r;
    if (!ix->opt.range_exact) {
        HIP_TRY(launch_range(P, (uint32_t)nq, ix->device, stream, ps.start(), ps.stop()));
        return RBQ_OK;
    }
    // r stays on the estimate's scale and bounds the work; x is compared with the exact score itself (distance < x, dot > x)
    P.queries = d_queries; P.query_dtype = ix->opt.query_dtype; P.raw = ix->raw.p; P.raw_dtype = ix->raw_dtype; P.n_raw = ix->n_raw;
    P.dim = ix->dim;
    std::memcpy(&P.X, &ix->opt.range_exact_radius_bits, 4);
    HIP_TRY(launch_range_exact(P, (uint32_t)nq, ix->device, stream, ps.start(), ps.stop()));
    return RBQ_OK;
}

namespace {
// range search on this handle?  (MSTG handles — RBQ_ROTATOR_NONE — never take it)
inline bool range_on(const Replica* ix) { return ix->opt.range_search && ix->rotator != 2; }

using rbq_host::PrepForm;
using rbq_host::RankRoute;
using rbq_host::SearchPlan;

// Front of a search on device pointers, enqueued on `stream`, shared by the top-k scan and the range scan: what `plan` says, in the
// order plan -> buffers -> the three parameter blocks -> launches (prep / latency front, ranking GEMM or exact ranking, selection).
int search_front(Replica* ix, Workspace* w, const SearchPlan& plan, const float* d_queries, uint64_t nq, uint32_t top_k,
                 const uint32_t* d_filter, uint64_t filter_nbits, rbq_diag* d_diag, hipStream_t stream) {
    const uint32_t D = ix->D, Dc = ix->Dc;
    const uint32_t nlist = (uint32_t)ix->n_lists;
    const uint32_t nprobe = plan.nprobe, smask = plan.stage_mask;
    const uint64_t wl_stride = plan.wl_stride;
    const bool f16 = plan.rank == RankRoute::f16;

    // ---- buffers ---------------------------------------------------------------------------------------------------------------
    int rc;
    if ((rc = w->rot.ensure(nq * D * 4))) return rc;
    if ((rc = w->lut.ensure(nq * (size_t)Dc * 4))) return rc;
    if ((rc = w->consts.ensure(nq * sizeof(QueryConsts)))) return rc;
    if ((rc = w->scores.ensure(nq * (size_t)nlist * 4))) return rc;
    if ((rc = w->probe.ensure(nq * (size_t)nprobe * sizeof(ProbeInfo)))) return rc;
    if ((rc = w->wl.ensure(nq * wl_stride * sizeof(StreamItem)))) return rc;
    if ((rc = w->nstream.ensure(nq * 4))) return rc;
    if ((rc = w->nvec.ensure(nq * 8))) return rc;
    if ((rc = w->dead_skipped.ensure(nq * 16))) return rc;
    if (plan.need_rot_hl && (rc = w->rot_hl.ensure(nq * D * 4))) return rc;
    if (plan.need_rank_planes && (rc = w->rank_planes.ensure((nq + nlist) * (size_t)D * 4))) return rc;
    if (plan.need_rot_f16 && (rc = w->rot_f16.ensure(nq * D * 2))) return rc;
    if (plan.need_rank_resid && (rc = w->rank_resid.ensure(nq * 4))) return rc;
    if (plan.need_key_window && (rc = w->key_window.ensure((size_t)nq * select_exact_np2(nprobe) * 8))) return rc;
    if (ix->opt.lazy_audit && (rc = w->audit_dead.ensure(nq * (size_t)(kAuditCap + 1) * 4))) return rc;
    if (ix->opt.ub_tap && (rc = w->head_ub.ensure(nq * (size_t)kHeadUbRow * 4))) return rc;
    unsigned long long* prof = (ix->profiling && ix->opt.profile_counters) ? (unsigned long long*)ix->prof.p : nullptr;

    // ---- the three parameter blocks ------------------------------------------------------------------------------------------------
    PrepParams pp = prep_params(*ix, ix->rot_blob, *w, d_queries, nq, ix->opt.query_dtype);
    RankParams pr; // what the latency kernel reads of the ranking: with its scorers the exact scores, else the rows to clear
    pr.metric = ix->metric; pr.cent = nullptr; pr.nlist = nlist; pr.D = D; pr.nq = (uint32_t)nq; pr.scores = nullptr;
    if (plan.lat_front()) {
        pr.cent = (const float*)ix->centroids.p; pr.scores = (float*)w->scores.p;
    } else {
        pp.rot_hl = plan.need_rot_hl ? (uint16_t*)w->rot_hl.p : nullptr;
        if (f16) { pp.rot_hl = (uint16_t*)w->rot_f16.p; pp.rank_resid = (float*)w->rank_resid.p; }
        pp.wg_prep = ix->opt.wg_prep;
        pr.ksplit = 1;
        // (a split-K GEMM follows: this kernel clears the score rows its parts are added to; launch_lat_front reads that off ksplit > 1)
        if (plan.prep == PrepForm::wg_zero) { pr.scores = (float*)w->scores.p; pr.ksplit = std::max(plan.ksplit, 2u); }
    }
    RankParams rp;
    rp.metric = ix->metric; rp.rot = (const float*)w->rot.p; rp.rot_hi = (const uint16_t*)w->rot_hl.p; rp.rot_lo = nullptr; rp.rot_hl = true;
    rp.cent = (const float*)ix->centroids.p; rp.cent_hi = (const uint16_t*)ix->cent_hl.p; rp.cent_lo = nullptr; rp.cent_hl = true;
    rp.consts = (const QueryConsts*)w->consts.p; rp.cnorm2 = (const float*)ix->cnorm2.p; rp.nq = (uint32_t)nq; rp.nlist = nlist; rp.D = D;
    rp.scores = (float*)w->scores.p; rp.split = plan.split_route(); rp.ksplit = plan.ksplit;
    if (f16) { rp.f16 = true; rp.rot_hi = (const uint16_t*)w->rot_f16.p; rp.cent_hi = (const uint16_t*)ix->cent_f16.p; }
    rp.big = plan.tile == 128; rp.wide = plan.tile == 256;
    // TEST ONLY: the same GEMM on planar copies of its operands (made below, before the GEMM)
    uint16_t* const pl = plan.planar ? (uint16_t*)w->rank_planes.p : nullptr; // rot hi | rot lo | cent hi | cent lo
    const size_t nr = (size_t)nq * D, nc = (size_t)nlist * D;
    if (pl) {
        rp.rot_hi = pl; rp.rot_lo = pl + nr; rp.rot_hl = false;
        rp.cent_hi = pl + 2 * nr; rp.cent_lo = pl + 2 * nr + nc; rp.cent_hl = false;
    }
    SelectParams sp;
    sp.scores = (float*)w->scores.p; sp.nq = (uint32_t)nq; sp.nlist = nlist; sp.nprobe = nprobe; sp.metric = ix->metric;
    sp.rot = (const float*)w->rot.p; sp.cent = (const float*)ix->centroids.p; sp.D = D; sp.consts = (const QueryConsts*)w->consts.p;
    if (f16) { sp.rank_resid = (const float*)w->rank_resid.p; sp.cnorm_max = ix->cnorm_max; sp.rc_max = ix->rc_max; }
    sp.cnorm2_max = ix->cnorm2_max; sp.list_gb0 = (const uint32_t*)ix->list_gb0.p; sp.list_n = (const uint32_t*)ix->list_n.p;
    sp.probe = (ProbeInfo*)w->probe.p; sp.wl = (StreamItem*)w->wl.p; sp.wl_stride = wl_stride; sp.nstream = (uint32_t*)w->nstream.p;
    sp.nvec = (unsigned long long*)w->nvec.p; sp.prof_total = prof; sp.fallback_count = (unsigned int*)ix->fallbacks.p;
    sp.force_fallback = ix->opt.force_rank_fallback ? 1 : 0; sp.bsum = (const BlockSummary*)ix->bsum.p;
    sp.cnorm2 = (const float*)ix->cnorm2.p; sp.lsum = (const BlockSummary*)ix->lsum.p; sp.bsumx = (const BlockSummaryEx*)ix->bsumx.p;
    sp.dead_skipped = (uint32_t*)w->dead_skipped.p; sp.top_k = top_k; sp.ex_bits = ix->ex_bits;
    sp.slack = ix->opt.slack;
    sp.numeric_variant = ix->opt.numeric_variant;
    // diagnostics: the lists the selection drops as a whole, the lazy selection's head candidates and their bounds
    // (rbq_debug_copy_workspace "audit_dead" / "head_ub"; cleared below, before the selection)
    sp.audit_dead = ix->opt.lazy_audit ? (uint32_t*)w->audit_dead.p : nullptr;
    sp.head_ub = ix->opt.ub_tap ? (uint32_t*)w->head_ub.p : nullptr;
    sp.lazy = plan.lazy ? 1 : 0;
    sp.filter = d_filter; sp.filter_nbits = filter_nbits; sp.ids = (const uint64_t*)ix->ids.p;
    sp.exact_members = d_diag ? 1 : 0;
    sp.fault_dead_all = ix->opt.lazy_fault_inject ? 1 : 0;
    sp.lut = (const uint8_t*)w->lut.p; sp.blocks = (const uint8_t*)ix->blocks.p; sp.ex_codes = (const uint8_t*)ix->ex.p;
    sp.f_add_ex = (const float*)ix->fadd_ex.p; sp.f_rescale_ex = (const float*)ix->fres_ex.p; sp.Dc = Dc;
    sp.head_exact = ix->opt.head_exact ? 1 : 0;
    sp.n_blocks = (uint32_t)ix->n_blocks;

    // ---- launches --------------------------------------------------------------------------------------------------------------
    if (smask & 1u) { // (the latency front runs under the full mask only)
        ProfScope ps(ix, 0, stream);
        if (plan.prep == PrepForm::prep || plan.prep == PrepForm::prep_wave) HIP_TRY(launch_prep(pp, ix->device, stream));
        else HIP_TRY(launch_lat_front(pp, pr, ix->device, stream));
    }
    if (ix->opt.lazy_audit) HIP_TRY(hipMemsetAsync(w->audit_dead.p, 0, nq * (size_t)(kAuditCap + 1) * 4, stream));
    if (ix->opt.ub_tap) HIP_TRY(hipMemsetAsync(w->head_ub.p, 0, nq * (size_t)kHeadUbRow * 4, stream));
    if (pl && (smask & 2u)) {
        HIP_TRY(launch_hl_planes((const uint16_t*)w->rot_hl.p, nq, D, pl, pl + nr, stream));
        HIP_TRY(launch_hl_planes((const uint16_t*)ix->cent_hl.p, nlist, D, pl + 2 * nr, pl + 2 * nr + nc, stream));
    }
    if ((smask & 2u) && plan.rank != RankRoute::none) {
        ProfScope ps(ix, 1, stream);
        if (plan.rank == RankRoute::exact) HIP_TRY(launch_rank_exact(rp, stream));
        else HIP_TRY(launch_rank_gemm(rp, ix->device, stream)); // approximate scores: one MFMA GEMM
    }
    if (smask & 4u) {
        ProfScope ps(ix, 2, stream);
        if (plan.exact_select) HIP_TRY(launch_select_exact(sp, ix->device, stream, plan.need_key_window ? (uint64_t*)w->key_window.p : nullptr));
        else HIP_TRY(launch_select_mfma(sp, ix->device, stream)); // shortlist + exact canonical scores + exact select
    }
    return RBQ_OK;
}

// Core: the plan, then the front, then the stage that reads its stream — the top-k scan, or the range scan while the option
// range_search is on.  `rerank`: the unpooled rerank (k_rerank over the returned ids) follows the scan
int search_core(Replica* ix, Workspace* w, const float* d_queries, uint64_t nq, uint32_t top_k, uint32_t nprobe_in,
                const uint32_t* d_filter, uint64_t filter_nbits, uint64_t* d_ids, float* d_scores, uint32_t* d_counts,
                rbq_diag* d_diag, hipStream_t stream, bool rerank) {
    const bool range = range_on(ix);
    const SearchPlan plan = search_plan(ix, w, nq, top_k, nprobe_in, d_filter != nullptr, d_diag != nullptr, range, /*mstg=*/false);
    int rc;
    if (range) {
        // top_k is the capacity of a query's output row; no heap exists, so the heap workspace's 8 GiB rule does not apply
        if (top_k > kTopKHardMax) return fail(RBQ_INVALID_CONFIG, "range search: the capacity of a query's row is at most 2^20");
        if ((rc = search_front(ix, w, plan, d_queries, nq, top_k, d_filter, filter_nbits, d_diag, stream))) return rc;
        if (plan.stage_mask & 8u)
            return range_stage(ix, w, d_queries, nq, plan.nprobe, top_k, plan.wl_stride, d_filter, filter_nbits, d_ids, d_scores, d_counts, d_diag, stream);
        return RBQ_OK;
    }
    // the 8 GiB bound is the global-memory heap's (top_k beyond what the LDS holds); calls whose heap lives in LDS need no workspace
    if (top_k > kTopKHardMax || (plan.heap_in_global && (uint64_t)nq * ((uint64_t)top_k + 1) * 8 > (8ull << 30)))
        return fail(RBQ_INVALID_CONFIG, "top_k too large for one call (top_k <= 2^20 and nq * top_k * 8 bytes of heap workspace <= 8 GiB)");
    if (rerank && top_k > 1024) return fail(RBQ_INVALID_CONFIG, "rerank supports top_k <= 1024");
    if ((rc = search_front(ix, w, plan, d_queries, nq, top_k, d_filter, filter_nbits, d_diag, stream))) return rc;
    if ((plan.stage_mask & 8u) && (rc = scan_stage(ix, w, plan, nq, plan.nprobe, top_k, plan.wl_stride, d_filter, filter_nbits, d_ids, d_scores, d_counts,
                                                   d_diag, /*mstg=*/false, plan.exact_select ? nullptr : (const uint32_t*)w->dead_skipped.p, stream)))
        return rc;
    if (rerank && !stage_probes()) // optional, default off: exact re-scoring of the returned ids against the attached raw vectors
        HIP_TRY(launch_rerank(d_queries, ix->opt.query_dtype, (uint32_t)nq, ix->dim, ix->raw.p, ix->raw_dtype, ix->n_raw, ix->metric, top_k, d_ids, d_scores,
                              d_counts, stream));
    return RBQ_OK;
}

// The search of one batch on device pointers (d_queries: nq rows of the handle's query_dtype behind the float pointer — only the
// preparation and the rerank's copy of the query read them).  With the rerank on and a pool above top_k (option rerank_pool) the pipeline above runs
// unchanged at top_k := pool into the workspace, with the diagnostics of that call, and k_rerank_pool writes the caller's top_k:
// the pool's entries by (exact score, rank in the pool).  Every bound on top_k is then the inner call's, on `pool`.
int search_device(Replica* ix, Workspace* w, const float* d_queries, uint64_t nq, uint32_t top_k, uint32_t nprobe,
                  const uint32_t* d_filter, uint64_t filter_nbits, uint64_t* d_ids, float* d_scores, uint32_t* d_counts,
                  rbq_diag* d_diag, hipStream_t stream) {
    if (range_on(ix)) {
        // the exact range search (option range_exact) decides a match by the raw rows: it runs with the rerank
        // on and only then — nothing is silently approximated.  rerank_pool is not read in range mode.
        if (ix->opt.range_exact) {
            if (!ix->rerank)
                return fail(RBQ_INVALID_CONFIG, ix->raw.p ? "exact range search needs the rerank on: set the option rerank 1 or range_exact 0"
                                                          : "exact range search needs raw vectors attached (rbq_index_set_rerank_vectors) or range_exact 0");
            return search_core(ix, w, d_queries, nq, top_k, nprobe, d_filter, filter_nbits, d_ids, d_scores, d_counts, d_diag, stream, /*rerank=*/false);
        }
        if (ix->rerank)
            return fail(RBQ_INVALID_CONFIG, "range search does not run with the rerank on: set the option rerank 0 or detach the vectors");
    }
    const uint32_t pool = ix->opt.rerank_pool;
    if (!ix->rerank || pool <= top_k)
        return search_core(ix, w, d_queries, nq, top_k, nprobe, d_filter, filter_nbits, d_ids, d_scores, d_counts, d_diag, stream, ix->rerank);
    int rc;
    if ((rc = w->rr_ids.ensure(nq * (size_t)pool * 8))) return rc;
    if ((rc = w->rr_est.ensure(nq * (size_t)pool * 4))) return rc;
    if ((rc = w->rr_counts.ensure(nq * 4))) return rc;
    if ((rc = search_core(ix, w, d_queries, nq, pool, nprobe, d_filter, filter_nbits, (uint64_t*)w->rr_ids.p, (float*)w->rr_est.p,
                          (uint32_t*)w->rr_counts.p, d_diag, stream, /*rerank=*/false)))
        return rc;
    if (stage_probes()) return RBQ_OK; // (the four stages of the inner call are what a probe reports)
    RerankPoolParams P;
    P.queries = d_queries; P.query_dtype = ix->opt.query_dtype; P.raw = ix->raw.p; P.raw_dtype = ix->raw_dtype; P.n_raw = ix->n_raw; P.nq = (uint32_t)nq; P.dim = ix->dim; P.metric = ix->metric;
    P.pool = pool; P.top_k = top_k; P.pool_ids = (const uint64_t*)w->rr_ids.p; P.pool_counts = (const uint32_t*)w->rr_counts.p;
    P.out_ids = d_ids; P.out_scores = d_scores; P.out_counts = d_counts;
    HIP_TRY(launch_rerank_pool(P, ix->device, stream));
    return RBQ_OK;
}

// rbq_search_batch on ONE replica.  The batch is cut into sub-batches of (by default) 1024 queries that travel through
// up to six lanes (stream + workspace + pinned staging each), so the stages of neighbouring sub-batches overlap on the
// GPU exactly like bench.py's device-resident batches do, and the host stages sub-batch j+1 while j runs.
//  * results: k_scan writes ids / scores / counts / diagnostics STRAIGHT into page-locked host memory (the caller's
//    buffers when they are page-locked — rbq_host_alloc / hipHostMalloc / hipHostRegister — else the lane's pinned
//    staging, handed over with one memcpy): 123 KB per 1024 queries, no D2H copy command in the queue;
//  * queries: page-locked caller buffers are DMA-ed as they are, pageable ones are staged through the lane's pinned
//    buffer in pieces (the DMA of piece i runs under the memcpy of piece i+1);
//  * one event per sub-batch, no stream synchronisation.
int search_host(Replica* ix, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t top_k, uint32_t nprobe,
                const uint32_t* filter_words, uint64_t filter_nbits, uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                rbq_diag* diag) {
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    using clk = std::chrono::steady_clock;
    const bool trace = ix->opt.host_trace != 0;
    double t_attr = 0, t_ws = 0, t_stage = 0, t_enq = 0, t_wait = 0, t_out = 0;
    auto tick = [&](clk::time_point& t0, double& acc) { if (trace) { const auto t1 = clk::now(); acc += std::chrono::duration<double, std::micro>(t1 - t0).count(); t0 = t1; } };
    clk::time_point tp = clk::now();
    // sub-batches shrink towards the end of the call (rbq_host_logic.hpp): the last one's kernel chain is what the caller waits for
    const std::vector<std::pair<uint64_t, uint64_t>> plan = rbq_host::subbatch_plan(nq, ix->opt.host_subbatch);
    const uint64_t nsub = plan.size();
    const rbq_host::QueryRows qr = query_rows(ix, query_dim); // every byte length and row offset on the queries below is its arithmetic
    const bool in_pinned = is_pinned_host_range(queries, qr.bytes(nq));
    // lanes, the zero-copy window, helpers, the short-chain scan: the call's decisions, with their measurements, in rbq_host_logic.hpp
    rbq_host::HostCallOptions hopt;
    hopt.host_lanes = ix->opt.host_lanes; hopt.host_zero_copy = ix->opt.host_zero_copy; hopt.host_stage_helpers = ix->opt.host_stage_helpers;
    const rbq_host::HostCallPlan call = rbq_host::host_call_plan(nq, in_pinned, qr.bytes(nq), nsub, hopt);
    const uint32_t nlanes = call.nlanes;
    bool out_pinned = !ix->rerank && is_pinned_host_range(out_ids, nq * top_k * 8) && is_pinned_host_range(out_scores, nq * top_k * 4) &&
                      is_pinned_host_range(out_counts, nq * 4) && (!diag || is_pinned_host_range(diag, nq * sizeof(rbq_diag)));
    // device-side addresses of page-locked caller buffers (identical under unified addressing; asked for, not assumed)
    uint64_t* c_ids = nullptr; float* c_scores = nullptr; uint32_t* c_counts = nullptr; rbq_diag* c_diag = nullptr;
    if (out_pinned) {
        if (hipHostGetDevicePointer((void**)&c_ids, out_ids, 0) != hipSuccess || hipHostGetDevicePointer((void**)&c_scores, out_scores, 0) != hipSuccess ||
            hipHostGetDevicePointer((void**)&c_counts, out_counts, 0) != hipSuccess ||
            (diag && hipHostGetDevicePointer((void**)&c_diag, diag, 0) != hipSuccess)) {
            (void)hipGetLastError();
            out_pinned = false;
        }
    }
    // page-locked queries are read by k_prep where they lie (device-side address of the caller's buffer)
    const bool zero_copy = call.zero_copy;
    const float* c_queries = nullptr;
    if (zero_copy && in_pinned && hipHostGetDevicePointer((void**)&c_queries, const_cast<float*>(queries), 0) != hipSuccess) {
        (void)hipGetLastError();
        c_queries = nullptr;
    }
    tick(tp, t_attr);
    std::vector<Workspace*> lanes;
    struct Give { Replica* ix; std::vector<Workspace*>& l; bool drained = false;
                  ~Give() { for (Workspace* w : l) { if (!drained) (void)hipStreamSynchronize(w->stream); give_ws(ix, w); } } } give{ix, lanes};
    for (uint32_t i = 0; i < nlanes; ++i) {
        Workspace* w = take_ws(ix);
        if (!w) return fail(RBQ_DEVICE, "cannot create workspace stream");
        lanes.push_back(w);
    }
    tick(tp, t_ws);
    int rc;
    const uint32_t* d_filter = nullptr;
    if (filter_words) {
        const size_t fb = (size_t)((filter_nbits + 31) / 32) * 4;
        Workspace* w0 = lanes[0];
        if ((rc = w0->filter.ensure(fb ? fb : 4))) return rc;
        if (fb) HIP_TRY(hipMemcpyAsync(w0->filter.p, filter_words, fb, hipMemcpyHostToDevice, w0->stream));
        HIP_TRY(hipEventRecord(w0->done, w0->stream));
        for (uint32_t i = 1; i < nlanes; ++i) HIP_TRY(hipStreamWaitEvent(lanes[i]->stream, w0->done, 0));
        d_filter = (const uint32_t*)w0->filter.p;
    }
    // hand the finished sub-batch j (in the lane's pinned buffer) to the caller's arrays
    auto deliver = [&](Workspace* w, uint64_t j) -> int {
        clk::time_point td = clk::now();
        HIP_TRY(hipEventSynchronize(w->done));
        tick(td, t_wait);
        if (out_pinned) return RBQ_OK;
        const uint64_t q0 = plan[j].first, n = plan[j].second;
        const OutPack op(n, top_k, diag != nullptr);
        const uint8_t* src = (const uint8_t*)w->h_out.p;
        std::memcpy(out_ids + q0 * top_k, src + op.o_ids, n * top_k * 8);
        std::memcpy(out_scores + q0 * top_k, src + op.o_scores, n * top_k * 4);
        std::memcpy(out_counts + q0, src + op.o_counts, n * 4);
        if (diag) std::memcpy(diag + q0, src + op.o_diag, n * sizeof(rbq_diag));
        tick(td, t_out);
        return RBQ_OK;
    };
    // pageable queries, every sub-batch on its own lane (nsub <= nlanes): the helpers stage sub-batches 1.. into their lanes' pinned
    // buffers while this thread stages and launches sub-batch 0
    std::atomic<int> staged[rbq_host::kMaxHelped];
    uint64_t n_helped = 0; // sub-batches 1 .. n_helped are staged by helpers
    auto wait_staged = [&staged](uint64_t j) { spin_until([&] { return staged[j].load(std::memory_order_acquire) != 0; }); };
    struct WaitHelpers { decltype(wait_staged)& wait; uint64_t& n; // (no job may outlive this frame: it writes the flags)
        ~WaitHelpers() { for (uint64_t j = 1; j <= n; ++j) wait(j); } } wait_helpers{wait_staged, n_helped};
    bool helpers = call.helpers;
    if (helpers) {
        // the helpers are published only once every thread of theirs runs (a half-started set used to stay installed, and
        // jobs posted to it could wait forever); if a thread cannot be created the call stages inline, like a small one does
        std::lock_guard<std::mutex> lk(ix->mu);
        if (!ix->stagers && !ix->stagers_failed) {
            std::unique_ptr<StagePool> sh(new (std::nothrow) StagePool());
            if (sh && sh->start()) ix->stagers = std::move(sh);
            else ix->stagers_failed = true;
        }
        helpers = ix->stagers != nullptr;
    }
    if (helpers) {
        for (uint64_t j = 1; j < nsub; ++j) {
            Workspace* wj = lanes[j];
            if ((rc = wj->h_in.ensure(qr.bytes(plan[j].second)))) return rc; // (jobs posted so far are awaited by wait_helpers)
            staged[j].store(0, std::memory_order_relaxed);
            ix->stagers->post(StageJob{wj->h_in.p, qr.at(queries, plan[j].first), qr.bytes(plan[j].second), &staged[j]});
            n_helped = j;
        }
    }
    for (uint64_t j = 0; j < nsub; ++j) {
        Workspace* w = lanes[j % nlanes];
        if (j >= nlanes && (rc = deliver(w, j - nlanes))) return rc;
        const uint64_t q0 = plan[j].first, n = plan[j].second;
        const OutPack op(n, top_k, diag != nullptr);
        const bool staged_in_hbm = !(c_queries || (zero_copy && !in_pinned)); // an H2D copy into the lane's device buffer
        if (staged_in_hbm && (rc = w->queries.ensure(qr.bytes(n)))) return rc;
        const float* src = qr.at(queries, q0);
        tp = clk::now();
        const float* d_q = (const float*)w->queries.p; // where k_prep reads this sub-batch
        if (c_queries) {
            d_q = qr.at(c_queries, q0);
        } else if (zero_copy && !in_pinned) { // pageable: one host copy into the lane's pinned buffer, read from there
            if (j >= 1 && j <= n_helped) { // staged by a helper: wait for its copy
                wait_staged(j);
            } else {
                if ((rc = w->h_in.ensure(qr.bytes(n)))) return rc;
                std::memcpy(w->h_in.p, src, qr.bytes(n));
            }
            float* hp = nullptr;
            HIP_TRY(hipHostGetDevicePointer((void**)&hp, w->h_in.p, 0));
            d_q = hp;
        } else if (in_pinned) {
            HIP_TRY(hipMemcpyAsync(w->queries.p, src, qr.bytes(n), hipMemcpyHostToDevice, w->stream));
        } else if (j >= 1 && j <= n_helped) { // pageable, staged by a helper: wait for its copy, one DMA
            wait_staged(j);
            HIP_TRY(hipMemcpyAsync(w->queries.p, w->h_in.p, qr.bytes(n), hipMemcpyHostToDevice, w->stream));
        } else {
            if ((rc = w->h_in.ensure(qr.bytes(n)))) return rc;
            const uint64_t piece = std::max<uint64_t>(64, (n + 3) / 4); // queries per piece
            for (uint64_t p0 = 0; p0 < n; p0 += piece) {
                const size_t off = qr.bytes(p0), len = qr.bytes(std::min(piece, n - p0));
                std::memcpy((uint8_t*)w->h_in.p + off, (const uint8_t*)src + off, len);
                HIP_TRY(hipMemcpyAsync((uint8_t*)w->queries.p + off, (const uint8_t*)w->h_in.p + off, len, hipMemcpyHostToDevice, w->stream));
            }
        }
        tick(tp, t_stage);
        uint64_t* k_ids; float* k_scores; uint32_t* k_counts; rbq_diag* k_diag; // where the kernels write
        if (out_pinned) {
            k_ids = c_ids + q0 * top_k; k_scores = c_scores + q0 * top_k; k_counts = c_counts + q0; k_diag = diag ? c_diag + q0 : nullptr;
        } else if (!ix->rerank) {
            if ((rc = w->h_out.ensure(op.total))) return rc;
            uint8_t* hp = nullptr;
            HIP_TRY(hipHostGetDevicePointer((void**)&hp, w->h_out.p, 0));
            k_ids = (uint64_t*)(hp + op.o_ids); k_scores = (float*)(hp + op.o_scores); k_counts = (uint32_t*)(hp + op.o_counts);
            k_diag = diag ? (rbq_diag*)(hp + op.o_diag) : nullptr;
        } else { // the rerank kernel re-reads the ids: keep them in HBM, one D2H copy afterwards
            if ((rc = w->out_pack.ensure(op.total))) return rc;
            uint8_t* dp = (uint8_t*)w->out_pack.p;
            k_ids = (uint64_t*)(dp + op.o_ids); k_scores = (float*)(dp + op.o_scores); k_counts = (uint32_t*)(dp + op.o_counts);
            k_diag = diag ? (rbq_diag*)(dp + op.o_diag) : nullptr;
        }
        // every sub-batch of a call below kHostWaveMinQueries takes the short-chain kernel
        w->latency_first = call.latency_first;
        w->call_nq = nq;
        rc = search_device(ix, w, d_q, n, top_k, nprobe, d_filter, filter_nbits, k_ids, k_scores, k_counts, k_diag, w->stream);
        w->latency_first = false;
        w->call_nq = 0;
        if (rc) return rc;
        if (ix->rerank) {
            if ((rc = w->h_out.ensure(op.total))) return rc;
            HIP_TRY(hipMemcpyAsync(w->h_out.p, w->out_pack.p, op.total, hipMemcpyDeviceToHost, w->stream));
        }
        HIP_TRY(hipEventRecord(w->done, w->stream));
        tick(tp, t_enq);
    }
    for (uint64_t j = nsub > nlanes ? nsub - nlanes : 0; j < nsub; ++j)
        if ((rc = deliver(lanes[j % nlanes], j))) return rc;
    give.drained = true; // every lane's last event has been waited for
    if (trace)
        std::fprintf(stderr, "[rbq host] nq=%llu sub=%llu lanes=%u pinned(in,out)=%d,%d us: attr %.1f ws %.1f stage %.1f enqueue %.1f wait %.1f copy-out %.1f\n",
                     (unsigned long long)nq, (unsigned long long)plan[0].second, nlanes, (int)in_pinned, (int)out_pinned, t_attr, t_ws, t_stage, t_enq, t_wait, t_out);
    return RBQ_OK;
}
} // namespace
} // namespace rbq_api

extern "C" {
// ---- search ---------------------------------------------------------------------------------------
int rbq_search_batch_device(const rbq_index* ch, const float* d_queries, uint64_t nq, uint32_t query_dim, uint32_t top_k,
                            uint32_t nprobe, const uint32_t* d_filter_words, uint64_t filter_nbits, uint64_t* d_out_ids,
                            float* d_out_scores, uint32_t* d_out_counts, rbq_diag* d_diag, void* hip_stream) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    rbq_index* h = const_cast<rbq_index*>(ch);
    int rc = check_query_args(h, query_dim);
    if (rc) return rc;
    if (nq == 0) return RBQ_OK;
    if (nq > 0x7fffffffull) return fail(RBQ_INVALID_CONFIG, "batch too large");
    if ((rc = check_query_pointer(h, d_queries))) return rc;
    Replica* ix = replica_of_pointer(h, d_queries);
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    hipStream_t s = (hipStream_t)hip_stream;
    if (top_k == 0) { // Ok(vec![]) for every query, src/ivf.rs:1792-1794
        HIP_TRY(hipMemsetAsync(d_out_counts, 0, nq * 4, s));
        return RBQ_OK;
    }
    return search_device(ix, stream_workspace(ix, s), d_queries, nq, top_k, nprobe, d_filter_words, filter_nbits, d_out_ids, d_out_scores,
                         d_out_counts, d_diag, s);
    RBQ_GUARD_END
}

int rbq_release_stream(rbq_index* h, void* hip_stream) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    if (!h) return fail(RBQ_INVALID_CONFIG, "null index");
    for (Replica* ix : h->reps) {
        Workspace* w = nullptr;
        {
            std::lock_guard<std::mutex> lk(ix->mu);
            auto it = ix->stream_ws.find((hipStream_t)hip_stream);
            if (it != ix->stream_ws.end()) { w = it->second; ix->stream_ws.erase(it); }
        }
        if (w) { DeviceGuard g(ix->device); delete w; }
    }
    return RBQ_OK;
    RBQ_GUARD_END
}

int rbq_search_batch(const rbq_index* ch, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t top_k,
                     uint32_t nprobe, const uint32_t* filter_words, uint64_t filter_nbits, uint64_t* out_ids,
                     float* out_scores, uint32_t* out_counts, rbq_diag* diag) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    rbq_index* h = const_cast<rbq_index*>(ch);
    int rc = check_query_args(h, query_dim);
    if (rc) return rc;
    if (nq == 0) return RBQ_OK;
    if (top_k == 0) {
        if (out_counts) std::memset(out_counts, 0, nq * 4);
        if (diag) std::memset(diag, 0, nq * sizeof(rbq_diag));
        return RBQ_OK;
    }
    if (!queries || !out_ids || !out_scores || !out_counts) return fail(RBQ_INVALID_CONFIG, "null buffer");
    if ((rc = check_query_pointer(h, queries))) return rc;
    const size_t R = h->reps.size();
    if (R == 1 || nq < 2 * R) return search_host(h->reps[0], queries, nq, query_dim, top_k, nprobe, filter_words, filter_nbits, out_ids,
                                                  out_scores, out_counts, diag);
    // N replicas: contiguous shards [r*nq/R, (r+1)*nq/R) (batch_search is a par_iter over queries, src/ivf.rs:1743-1752);
    // replica 0 is served by the calling thread, replica r > 0 by its persistent worker thread; results land straight in
    // the caller's arrays, no exchange between devices
    {
        std::lock_guard<std::mutex> lk(h->worker_mu);
        while (h->workers.size() + 1 < R) { // (published only once every thread of theirs runs)
            std::unique_ptr<ReplicaPool> w(new ReplicaPool());
            if (!w->start()) return fail(RBQ_IO, "cannot start the worker threads of a replica");
            h->workers.push_back(std::move(w));
        }
    }
    // Everything the posted jobs touch lives in one shared state they hold by value: a job that is still running when this
    // frame unwinds (post() threw after earlier replicas were posted) writes into memory it co-owns, never into a dead stack.
    struct ShardState {
        std::mutex mu; std::condition_variable cv; size_t left = 0;
        std::vector<int> rcs; std::vector<std::string> details;
    };
    auto st = std::make_shared<ShardState>();
    st->rcs.assign(R, RBQ_OK);
    st->details.resize(R);
    st->left = R - 1;
    auto shard = [st, h, R, nq, queries, query_dim, top_k, nprobe, filter_words, filter_nbits, out_ids, out_scores, out_counts, diag](size_t r) {
        uint64_t q0, q1;
        rbq_host::shard_range(r, R, nq, &q0, &q1);
        try {
            st->rcs[r] = search_host(h->reps[r], query_rows(h->reps[r], query_dim).at(queries, q0), q1 - q0, query_dim, top_k, nprobe, filter_words, filter_nbits,
                                     out_ids + q0 * top_k, out_scores + q0 * top_k, out_counts + q0, diag ? diag + q0 : nullptr);
        } catch (...) { st->rcs[r] = RBQ_IO; g_err = "internal error"; }
        st->details[r] = g_err; // thread-local in the worker
    };
    size_t posted = 0;
    bool post_failed = false;
    try {
        for (size_t r = 1; r < R; ++r) {
            h->workers[r - 1]->post([st, shard, r] {
                shard(r);
                std::lock_guard<std::mutex> lk(st->mu);
                if (--st->left == 0) st->cv.notify_one();
            });
            ++posted;
        }
    } catch (...) { post_failed = true; }
    if (post_failed) { // the caller's buffers must stay valid until the shards already under way have finished
        std::unique_lock<std::mutex> lk(st->mu);
        st->left -= (R - 1 - posted);
        st->cv.wait(lk, [&] { return st->left == 0; });
        return fail(RBQ_IO, "out of host memory");
    }
    shard(0);
    {
        // the other shards finish about when this one does: poll briefly before blocking on the latch
        const auto t0 = std::chrono::steady_clock::now();
        std::unique_lock<std::mutex> lk(st->mu);
        while (st->left != 0) {
            if (std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(200)) { lk.unlock(); std::this_thread::yield(); lk.lock(); }
            else st->cv.wait(lk, [&] { return st->left == 0; });
        }
    }
    for (size_t r = 0; r < R; ++r) if (st->rcs[r]) return fail(st->rcs[r], st->details[r]);
    return RBQ_OK;
    RBQ_GUARD_END
}

// Which kernel instantiation each of the four stages launches for a call of this shape, and what it occupies.
// out[stage][6] = workgroups, threads per workgroup, VGPRs per lane, LDS bytes per workgroup (static + dynamic), scratch bytes per
// lane, operand format (rank: kRankOps* — 1 split-bf16, 2 one f16 product, 3 f32; else 0); stages in the order prep, rank, select, scan.
// Nothing is launched.
int rbq_debug_stage_resources(rbq_index* h, uint64_t nq, uint32_t top_k, uint32_t nprobe, uint32_t* out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    if (!h || h->reps.empty() || !out || nq == 0 || nq > 0x7fffffffull || top_k == 0) return fail(RBQ_INVALID_CONFIG, "bad argument");
    Replica* ix = h->reps[0];
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    Workspace w; // scratch buffers are sized like a real call's (and freed on return); no kernel runs
    StageProbes probes;
    int rc;
    {
        // the probe comes off this thread on EVERY exit path (an exception out of search_device — bad_alloc from a
        // workspace — used to leave it installed, and every later search of the thread then launched nothing and returned RBQ_OK)
        struct ProbeGuard { ProbeGuard(StageProbes* p) { stage_probes() = p; } ~ProbeGuard() { stage_probes() = nullptr; } } guard(&probes);
        rc = search_device(ix, &w, nullptr, nq, top_k, nprobe, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
    }
    if (rc) return rc;
    for (int st = 0; st < 4; ++st) {
        const KernelProbe& k = probes.k[st];
        hipFuncAttributes fa;
        uint32_t* o = out + 6 * st;
        if (!k.fn) { // a stage this call shape does not launch (the latency-first front of a small call covers prep AND rank): zeros
            if (st != 1) return fail(RBQ_DEVICE, "stage was not probed");
            for (int j = 0; j < 6; ++j) o[j] = 0;
            o[5] = kRankOpsF32; // (the front's exact scores)
            continue;
        }
        HIP_TRY(hipFuncGetAttributes(&fa, k.fn));
        o[0] = k.grid_x * (k.grid_y ? k.grid_y : 1u) * (k.grid_z ? k.grid_z : 1u); // (z: the parts of a split-K GEMM)
        o[1] = k.block; o[2] = (uint32_t)fa.numRegs;
        o[3] = (uint32_t)(fa.sharedSizeBytes + k.dyn_lds); o[4] = (uint32_t)fa.localSizeBytes; o[5] = k.operands;
    }
    return RBQ_OK;
    RBQ_GUARD_END
}
} // extern "C"
