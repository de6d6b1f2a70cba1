// api_mstg_search.hip — MSTG search: the posting-list scan over lists the caller chose (rbq_posting_scan_batch) and the search in
// one call, plain or refined, on host or device buffers (rbq_mstg_search_*batch*, include/rbq_mstg.h).  The scan itself is api_search.hip's scan_stage.
#include <optional>

#include "api.hpp"
#include "rbq_mstg.h"

using namespace rbq_api;

namespace rbq_api {
namespace {
// ---- what the posting-list scan and the search share ---------------------------------------------------------------------------
// Stage 0: rotated queries, LUTs and query constants of n queries at d_q.  MSTG search never evaluates the ex codes, so they are
// prepared with ex_bits 0; the refined search keeps the handle's ex_bits: kbx, scale and the ex-dot range of the query constants
// follow it, and nothing the binary stage reads does.
int mstg_prep(Replica* ix, Workspace* w, const float* d_q, uint64_t n, bool keep_ex_bits, hipStream_t stream) {
    int rc;
    if ((rc = w->rot.ensure(n * ix->D * 4))) return rc;
    if ((rc = w->lut.ensure(n * (size_t)ix->Dc * 4))) return rc;
    if ((rc = w->consts.ensure(n * sizeof(QueryConsts)))) return rc;
    ProfScope ps(ix, 0, stream);
    PrepParams p = prep_params(*ix, ix->rot_blob, *w, d_q, n, ix->opt.query_dtype);
    if (!keep_ex_bits) p.ex_bits = 0u;
    HIP_TRY(launch_prep(p, ix->device, stream));
    return RBQ_OK;
}

// Stages 2 and 3 over the lists d_lists [n][list_stride] / d_lcnt [n] (device) of n prepared queries: the probes and work lists, then
// the scan.  d_slot_map (or null): the scan names its candidates through this map instead of the ids (the refined search).
int scan_posting_lists(Replica* ix, Workspace* w, uint64_t n, const uint32_t* d_lists, const uint32_t* d_lcnt, uint32_t list_stride,
                       uint64_t wl_stride, uint32_t top_k, uint64_t* d_ids, float* d_scores, uint32_t* d_counts, const uint64_t* d_slot_map,
                       hipStream_t stream) {
    int rc;
    if ((rc = w->probe.ensure(n * (size_t)list_stride * sizeof(ProbeInfo)))) return rc;
    if ((rc = w->wl.ensure(n * wl_stride * sizeof(StreamItem)))) return rc;
    if ((rc = w->nstream.ensure(n * 4))) return rc;
    {
        ProfScope ps(ix, 2, stream);
        ProbesGivenParams p;
        p.list_ids = d_lists; p.list_counts = d_lcnt; p.max_lists = list_stride;
        p.nq = (uint32_t)n; p.nlist = (uint32_t)ix->n_lists; p.metric = (int)ix->metric; p.rot = (const float*)w->rot.p;
        p.cent = (const float*)ix->centroids.p; p.D = ix->D; p.list_gb0 = (const uint32_t*)ix->list_gb0.p;
        p.list_n = (const uint32_t*)ix->list_n.p; p.probe = (ProbeInfo*)w->probe.p; p.wl = (StreamItem*)w->wl.p;
        p.wl_stride = wl_stride; p.nstream = (uint32_t*)w->nstream.p; p.consts = (const QueryConsts*)w->consts.p;
        p.bsum = (const BlockSummary*)ix->bsum.p;
        p.numeric_variant = ix->opt.numeric_variant;
        HIP_TRY(launch_probes_given(p, stream));
    }
    const rbq_host::SearchPlan plan = search_plan(ix, w, n, top_k, list_stride, false, false, /*range=*/false, /*mstg=*/true);
    return scan_stage(ix, w, plan, n, list_stride, top_k, wl_stride, nullptr, 0, d_ids, d_scores, d_counts, nullptr, /*mstg=*/true, nullptr,
                      stream, d_slot_map);
}

// A host call in chunks on the pool workspace w: each chunk's queries are uploaded, body(q0, n, d_q, d_ids, d_scores, d_counts, stream)
// enqueues its work, and its three result arrays are downloaded and waited for.  w returns to the pool on every path (after an
// error only once its stream has drained: queued work may still use its buffers).
template <class Body>
int host_chunks(Replica* ix, Workspace* w, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t top_k, uint64_t chunk,
                uint64_t* out_ids, float* out_scores, uint32_t* out_counts, Body body) {
    const rbq_host::QueryRows qr = query_rows(ix, query_dim);
    auto run = [&]() -> int {
        int rc;
        hipStream_t st = w->stream;
        for (uint64_t q0 = 0; q0 < nq; q0 += chunk) {
            const uint64_t n = std::min(chunk, nq - q0);
            const OutPack op(n, top_k, false);
            if ((rc = w->queries.ensure(qr.bytes(n)))) return rc;
            if ((rc = w->out_pack.ensure(op.total))) return rc;
            uint8_t* dp = (uint8_t*)w->out_pack.p;
            HIP_TRY(hipMemcpyAsync(w->queries.p, qr.at(queries, q0), qr.bytes(n), hipMemcpyHostToDevice, st));
            if ((rc = body(q0, n, (const float*)w->queries.p, (uint64_t*)(dp + op.o_ids), (float*)(dp + op.o_scores), (uint32_t*)(dp + op.o_counts), st)))
                return rc;
            HIP_TRY(hipMemcpyAsync(out_ids + q0 * top_k, dp + op.o_ids, n * top_k * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(out_scores + q0 * top_k, dp + op.o_scores, n * top_k * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(out_counts + q0, dp + op.o_counts, n * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        return RBQ_OK;
    };
    const int rc = run();
    if (rc) (void)hipStreamSynchronize(w->stream);
    give_ws(ix, w);
    return rc;
}

// the host-side result of a call without candidates: every count 0, every slot unused
void no_candidates(uint64_t nq, uint32_t top_k, uint64_t* out_ids, float* out_scores, uint32_t* out_counts) {
    std::memset(out_counts, 0, nq * 4);
    for (uint64_t i = 0; i < nq * top_k; ++i) { out_ids[i] = ~0ull; out_scores[i] = NAN; }
}

// ---- MSTG search (include/rbq_mstg.h): centroid ranking and dynamic_prune on the device, then the posting-list scan -------
constexpr uint64_t kMstgSearchBudget = 1ull << 30; // per-chunk workspace of rbq_mstg_search_batch* (option mstg_search_budget)
std::mutex g_ms_mu;
unsigned long long* g_ms_fallbacks[16] = {}; // per device: queries scored against every centroid (never freed)

// the counter of the current device `dev`
int ms_fallback_counter(int dev, unsigned long long** out) {
    std::lock_guard<std::mutex> lk(g_ms_mu);
    if (dev < 0 || dev >= 16) return fail(RBQ_DEVICE, "device ordinal out of range");
    if (!g_ms_fallbacks[dev]) {
        unsigned long long* p = nullptr;
        HIP_TRY(hipMalloc(&p, 8));
        if (hipMemset(p, 0, 8) != hipSuccess) { (void)hipFree(p); return fail(RBQ_DEVICE, "hipMemset failed"); }
        g_ms_fallbacks[dev] = p;
    }
    *out = g_ms_fallbacks[dev];
    return RBQ_OK;
}

// the centroids as the list selection sees them: ms_nc holds nc [k] | ncmax bits | the non-finite flag (images: GEMM shapes only)
CentView ms_view(const Replica* ix) {
    const uint32_t k = (uint32_t)ix->n_lists;
    return {k, ix->D, km_dp(ix->D), (float*)ix->ms_nc.p, (uint32_t*)ix->ms_nc.p + k, (uint16_t*)ix->ms_hi.p, (uint16_t*)ix->ms_lo.p};
}

// split-bf16 images and norms of the centroids, once per replica (the first search that takes the GEMM shortlist)
int ms_prepare(Replica* ix) {
    std::lock_guard<std::mutex> lk(ix->mu);
    if (ix->ms_ready) return RBQ_OK;
    const uint32_t k = (uint32_t)ix->n_lists, Dp = km_dp(ix->D);
    int rc;
    if ((rc = alloc_arr(ix->ms_hi, (size_t)k * Dp * 2))) return rc;
    if ((rc = alloc_arr(ix->ms_lo, (size_t)k * Dp * 2))) return rc;
    if ((rc = alloc_arr(ix->ms_nc, (size_t)k * 4 + 8))) return rc;
    const CentView cv = ms_view(ix);
    bool bad = false;
    HIP_TRY(launch_split_centroids((const float*)ix->centroids.p, cv, nullptr));
    HIP_TRY(nonfinite_sync((const float*)ix->centroids.p, (uint64_t)k * ix->D, cv.ncmax_bits + 1, nullptr, &bad));
    ix->ms_bad = bad;
    ix->ms_ready = true;
    return RBQ_OK;
}

// the refined search's identity slot map and list of every block, once per replica (the first refined search waits for them)
int mr_prepare(Replica* ix) {
    std::lock_guard<std::mutex> lk(ix->mu);
    if (ix->mr_ready) return RBQ_OK;
    int rc;
    if ((rc = alloc_arr(ix->mr_slot_map, (size_t)ix->n_blocks * 32 * 8))) return rc;
    if ((rc = alloc_arr(ix->mr_blk_list, (size_t)ix->n_blocks * 4))) return rc;
    HIP_TRY(launch_mstg_refine_maps((const uint32_t*)ix->list_gb0.p, (const uint32_t*)ix->list_n.p, (uint32_t)ix->n_lists, (uint32_t)ix->n_blocks,
                                    (uint64_t*)ix->mr_slot_map.p, (uint32_t*)ix->mr_blk_list.p, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    ix->mr_ready = true;
    return RBQ_OK;
}

struct MstgShape {
    uint32_t ef;        // min(ef_search, n_lists) >= 1: the stride of the list rows
    uint64_t wl_stride; // the ef longest lists together, in blocks
    uint64_t chunk;     // queries per pass
};

// The chunk keeps the work list and the score matrix inside the budget; the result does not depend on it.
// pool: the candidates per query of the refined search (0: the plain search), whose slots, estimates and counts join the chunk
MstgShape ms_shape(const Replica* ix, uint64_t nq, uint32_t top_k, uint32_t ef_search, bool host, uint32_t pool) {
    MstgShape sh;
    const uint64_t k = ix->n_lists;
    sh.ef = (uint32_t)std::min<uint64_t>(ef_search, k);
    sh.wl_stride = std::max<uint64_t>(ix->nblk_desc_prefix[sh.ef], 1);
    uint64_t per = (uint64_t)ix->D * 4 + (uint64_t)ix->Dc * 4 + sizeof(QueryConsts) + (uint64_t)sh.ef * (4 + sizeof(ProbeInfo)) +
                   sh.wl_stride * sizeof(StreamItem) + (uint64_t)top_k * 12 + 16;
    if (host) per += (uint64_t)ix->dim * 4;
    if (pool) per += (uint64_t)pool * 12 + 4;
    if (mstg_select_gemm(k, ix->D)) per += gemm_shortlist_row_bytes(k, km_dp(ix->D), kMsCap) + 4; // (+ the query's norm)
    else if (k > RBQ_MSTG_SHORTLIST) per += 4;
    per += 8ull * mstg_select_knp2(k);
    const uint64_t budget = ix->opt.mstg_search_budget ? ix->opt.mstg_search_budget : kMstgSearchBudget;
    sh.chunk = std::min<uint64_t>(std::min<uint64_t>(std::max<uint64_t>(budget / per, 1), 16384), nq);
    return sh;
}

// What an entry point was called with; the buffers are the host's or the device's alike.
struct MstgArgs {
    const float* queries; uint64_t nq; uint32_t query_dim, top_k, ef_search; float pruning_epsilon;
    uint64_t* out_ids; float* out_scores; uint32_t* out_counts; uint32_t* out_list_ids; uint32_t* out_list_counts;
    bool refined = false;     // rbq_mstg_search_refined_batch*: the pool is max(refine_pool, top_k)
    uint32_t refine_pool = 0;
};

// One search call once mstg_begin has checked and prepared it: what every chunk of it needs.
struct MstgCall {
    bool done = true;         // answered by mstg_begin (an error, no query or no candidate): nothing to run
    Replica* ix = nullptr;
    std::optional<DeviceGuard> guard; // the replica's device for as long as the call lives
    uint32_t top_k = 0, ef_search = 0;
    float pruning_epsilon = 0;
    uint32_t pool = 0;        // candidates per query that the refined search scans for and refines (0: the plain search)
    bool exact = false;       // option mstg_rerank on a refined call: the pool is scored against the raw rows (k_mstg_rerank.hip)
    unsigned long long* d_fallbacks = nullptr;
    MstgShape sh{};
};

// the argument errors of the MSTG searches (rbq_host::mstg_search_check: what rbq_posting_scan_batch checks, in its order, then
// the refined call's pool); *pool = max(refine_pool, top_k) of a refined call
int ms_check(const rbq_index* h, const MstgArgs& c, uint32_t* pool) {
    static_assert(rbq_host::kMstgTopKHardMax == kTopKHardMax && rbq_host::kMstgRefinePoolMax == RBQ_MSTG_REFINE_POOL_MAX, "host logic and device side disagree");
    rbq_host::MstgSearchArgs a;
    a.have_index = h && !h->reps.empty();
    if (a.have_index) { const Replica* ix = h->reps[0]; a.n_vectors = ix->n_vectors; a.dim = ix->dim; a.rotator = ix->rotator; }
    a.query_dim = c.query_dim; a.nq = c.nq; a.top_k = c.top_k; a.refined = c.refined; a.refine_pool = c.refine_pool;
    a.queries = c.queries != nullptr; a.out_ids = c.out_ids != nullptr; a.out_scores = c.out_scores != nullptr; a.out_counts = c.out_counts != nullptr;
    std::string detail;
    bool done = false;
    const int rc = rbq_host::mstg_search_check(a, &detail, &done, pool);
    return rc ? fail(rc, detail) : RBQ_OK;
}

// Everything both entries do before the first chunk: the argument errors, the replica and its device, the answer of a call without
// candidates (host: plain stores, before the device is touched; else enqueued on s), the one-time preparations, the shape.
int mstg_begin(rbq_index* h, const MstgArgs& a, bool host, hipStream_t s, MstgCall* c) {
    int rc = ms_check(h, a, &c->pool);
    if (rc || a.nq == 0) return rc;
    if ((rc = check_query_pointer(h, a.queries))) return rc;
    Replica* ix = c->ix = host ? h->reps[0] : replica_of_pointer(h, a.queries);
    if (a.refined) { // the exact rerank of the pool reads the raw rows of the replica that serves the call, or the call is refused
        std::string detail;
        if ((rc = rbq_host::mstg_rerank_check(ix->opt.mstg_rerank, ix->raw.p != nullptr && ix->n_raw != 0, ix->rerank, &detail))) return fail(rc, detail);
        c->exact = ix->opt.mstg_rerank;
    }
    const uint32_t ef = (uint32_t)std::min<uint64_t>(a.ef_search, ix->n_lists);
    const bool empty = a.top_k == 0 || ef == 0;
    if (host && empty) {
        no_candidates(a.nq, a.top_k, a.out_ids, a.out_scores, a.out_counts);
        if (a.out_list_counts) std::memset(a.out_list_counts, 0, a.nq * 4);
        if (a.out_list_ids) std::memset(a.out_list_ids, 0xff, a.nq * (size_t)ef * 4);
        return RBQ_OK;
    }
    c->guard.emplace(ix->device);
    if (!c->guard->ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    if (empty) { // (all-ones words: UINT64_MAX ids, UINT32_MAX lists, NaN scores)
        HIP_TRY(hipMemsetAsync(a.out_counts, 0, a.nq * 4, s));
        if (a.out_list_counts) HIP_TRY(hipMemsetAsync(a.out_list_counts, 0, a.nq * 4, s));
        if (a.out_list_ids && ef) HIP_TRY(hipMemsetAsync(a.out_list_ids, 0xff, a.nq * (size_t)ef * 4, s));
        if (a.top_k) {
            HIP_TRY(hipMemsetAsync(a.out_ids, 0xff, a.nq * (size_t)a.top_k * 8, s));
            HIP_TRY(hipMemsetAsync(a.out_scores, 0xff, a.nq * (size_t)a.top_k * 4, s));
        }
        return RBQ_OK;
    }
    if (mstg_select_gemm(ix->n_lists, ix->D) && (rc = ms_prepare(ix))) return rc;
    if ((rc = ms_fallback_counter(ix->device, &c->d_fallbacks))) return rc;
    if (a.refined && (rc = mr_prepare(ix))) return rc; // (the first refined call on a handle waits for its maps once)
    c->top_k = a.top_k; c->ef_search = a.ef_search; c->pruning_epsilon = a.pruning_epsilon;
    c->sh = ms_shape(ix, a.nq, a.top_k, a.ef_search, host, c->pool);
    if (c->sh.wl_stride > 0xffffffffull) return fail(RBQ_INVALID_CONFIG, "posting lists too long for one query");
    c->done = false;
    return RBQ_OK;
}

// n queries at d_q (device; rows of the handle's query_dtype, read by mstg_prep alone), everything enqueued on `stream`; d_lists [n][sh.ef] and d_lcnt [n] receive the selection.
// Refined (c.pool, k_mstg_refine.hip): the scan runs with top_k := pool over the slot map into the workspace's pool, which is
// then refined into the caller's top_k — with the ex codes, or (c.exact, k_mstg_rerank.hip) exactly against the raw rows, for
// which d_q is read once more, as the caller's rows in input space.
int run_chunk(const MstgCall& c, Workspace* w, const float* d_q, uint64_t n, uint64_t* d_ids, float* d_scores, uint32_t* d_counts,
              uint32_t* d_lists, uint32_t* d_lcnt, hipStream_t stream) {
    int rc;
    Replica* ix = c.ix;
    const MstgShape& sh = c.sh;
    uint64_t* s_ids = d_ids; float* s_scores = d_scores; uint32_t* s_counts = d_counts; // where the scan writes
    if (c.pool) {
        if ((rc = w->mr_pool.ensure(n * ((size_t)c.pool * 12 + 4)))) return rc;
        s_ids = (uint64_t*)w->mr_pool.p;
        s_scores = (float*)(s_ids + n * (size_t)c.pool);
        s_counts = (uint32_t*)(s_scores + n * (size_t)c.pool);
    }
    const uint32_t D = ix->D, k = (uint32_t)ix->n_lists, Dp = km_dp(D);
    const bool gemm = mstg_select_gemm(k, D);
    const uint64_t np = (n + 127) / 128 * 128; // (the GEMM's row tiles)
    if ((rc = w->ms_sl.ensure(n * ((size_t)(gemm ? kMsCap : 0) + 2) * 4))) return rc; // sl [n][kMsCap] | sl_n [n] | nx [n]
    if (gemm) {
        if ((rc = w->scores.ensure(np * (size_t)k * 4))) return rc;
        if ((rc = w->rot_hl.ensure(np * (size_t)Dp * 4))) return rc; // (here as two planes [np][Dp]: launch_approx_dots')
    }
    const uint32_t knp2 = mstg_select_knp2(k);
    if (knp2 && (rc = w->key_window.ensure(n * (size_t)knp2 * 8))) return rc;
    if ((rc = mstg_prep(ix, w, d_q, n, /*keep_ex_bits=*/c.pool != 0 && !c.exact, stream))) return rc; // (the exact rerank reads no ex code)
    {
        ProfScope ps(ix, 1, stream);
        MstgSelectParams p{};
        p.rot = (const float*)w->rot.p; p.nq = (uint32_t)n; p.ef_search = c.ef_search; p.pruning_epsilon = c.pruning_epsilon;
        p.cent = (const float*)ix->centroids.p; p.cv = ms_view(ix); p.cent_bad = ix->ms_bad;
        p.q_hi = (uint16_t*)w->rot_hl.p; p.q_lo = p.q_hi + np * (size_t)Dp;
        p.sl = (uint32_t*)w->ms_sl.p; p.sl_n = p.sl + n * (size_t)(gemm ? kMsCap : 0); p.nx = (float*)(p.sl_n + n);
        p.dots = (float*)w->scores.p; p.keys_g = knp2 ? (unsigned long long*)w->key_window.p : nullptr;
        p.fallbacks = c.d_fallbacks; p.out_lists = d_lists; p.out_counts = d_lcnt;
        HIP_TRY(launch_mstg_select(p, ix->device, stream));
    }
    rc = scan_posting_lists(ix, w, n, d_lists, d_lcnt, sh.ef, sh.wl_stride, c.pool ? c.pool : c.top_k, s_ids, s_scores, s_counts,
                            c.pool ? (const uint64_t*)ix->mr_slot_map.p : nullptr, stream);
    if (rc || !c.pool) return rc;
    uint32_t pool_np2 = 1;
    while (pool_np2 < c.pool) pool_np2 <<= 1;
    if (c.exact) {
        MstgRerankParams X{};
        X.ids = (const uint64_t*)ix->ids.p; X.blk_list = (const uint32_t*)ix->mr_blk_list.p; X.n_slots = ix->n_blocks * 32;
        X.probe = (const ProbeInfo*)w->probe.p; X.list_counts = d_lcnt; X.probe_stride = sh.ef;
        X.pool_slots = s_ids; X.pool_scores = s_scores; X.pool_counts = s_counts; X.pool = c.pool; X.pool_np2 = pool_np2;
        X.queries = d_q; X.query_dtype = ix->opt.query_dtype; X.raw = ix->raw.p; X.raw_dtype = ix->raw_dtype; X.n_raw = ix->n_raw;
        X.out_ids = d_ids; X.out_scores = d_scores; X.out_counts = d_counts;
        X.nq = (uint32_t)n; X.dim = ix->dim; X.metric = ix->metric; X.top_k = c.top_k;
        HIP_TRY(launch_mstg_rerank(X, ix->device, stream));
        return RBQ_OK;
    }
    MstgRefineParams P{};
    P.blocks = (const uint8_t*)ix->blocks.p; P.ids = (const uint64_t*)ix->ids.p; P.ex_codes = (const uint8_t*)ix->ex.p;
    P.f_add_ex = (const float*)ix->fadd_ex.p; P.f_rescale_ex = (const float*)ix->fres_ex.p;
    P.blk_list = (const uint32_t*)ix->mr_blk_list.p; P.n_slots = ix->n_blocks * 32;
    P.lut = (const uint8_t*)w->lut.p; P.rot = (const float*)w->rot.p; P.consts = (const QueryConsts*)w->consts.p;
    P.probe = (const ProbeInfo*)w->probe.p; P.list_counts = d_lcnt; P.probe_stride = sh.ef;
    P.pool_slots = s_ids; P.pool_scores = s_scores; P.pool_counts = s_counts; P.pool = c.pool;
    P.pool_np2 = pool_np2;
    P.out_ids = d_ids; P.out_scores = d_scores; P.out_counts = d_counts;
    P.nq = (uint32_t)n; P.D = D; P.Dc = ix->Dc; P.ex_bits = ix->ex_bits; P.metric = ix->metric; P.top_k = c.top_k;
    P.numeric_variant = ix->opt.numeric_variant;
    HIP_TRY(launch_mstg_refine(P, ix->device, stream));
    return RBQ_OK;
}

int ms_search_host(const rbq_index* ch, const MstgArgs& a) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    MstgCall c;
    const int rc = mstg_begin(const_cast<rbq_index*>(ch), a, /*host=*/true, nullptr, &c);
    if (rc || c.done) return rc;
    Workspace* w = take_ws(c.ix);
    if (!w) return fail(RBQ_DEVICE, "cannot create workspace stream");
    return host_chunks(c.ix, w, a.queries, a.nq, a.query_dim, a.top_k, c.sh.chunk, a.out_ids, a.out_scores, a.out_counts,
                       [&](uint64_t q0, uint64_t n, const float* d_q, uint64_t* d_ids, float* d_scores, uint32_t* d_counts, hipStream_t st) -> int {
        int r2;
        if ((r2 = w->ms_lists.ensure(n * ((size_t)c.sh.ef + 1) * 4))) return r2;
        uint32_t* d_lists = (uint32_t*)w->ms_lists.p;
        uint32_t* d_lcnt = d_lists + n * (size_t)c.sh.ef;
        if ((r2 = run_chunk(c, w, d_q, n, d_ids, d_scores, d_counts, d_lists, d_lcnt, st))) return r2;
        if (a.out_list_ids) HIP_TRY(hipMemcpyAsync(a.out_list_ids + q0 * c.sh.ef, d_lists, n * (size_t)c.sh.ef * 4, hipMemcpyDeviceToHost, st));
        if (a.out_list_counts) HIP_TRY(hipMemcpyAsync(a.out_list_counts + q0, d_lcnt, n * 4, hipMemcpyDeviceToHost, st));
        return RBQ_OK;
    });
    RBQ_GUARD_END
}

int ms_search_device(const rbq_index* ch, const MstgArgs& a, void* hip_stream) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    hipStream_t s = (hipStream_t)hip_stream;
    MstgCall c;
    int rc = mstg_begin(const_cast<rbq_index*>(ch), a, /*host=*/false, s, &c);
    if (rc || c.done) return rc;
    const MstgShape& sh = c.sh;
    Workspace* w = stream_workspace(c.ix, s); // (as rbq_search_batch_device: the chunks of a call and successive calls are stream-ordered)
    const bool own_lists = !a.out_list_ids || !a.out_list_counts;
    if (own_lists && (rc = w->ms_lists.ensure(sh.chunk * ((size_t)sh.ef + 1) * 4))) return rc;
    for (uint64_t q0 = 0; q0 < a.nq; q0 += sh.chunk) {
        const uint64_t n = std::min(sh.chunk, a.nq - q0);
        uint32_t* d_lists = a.out_list_ids ? a.out_list_ids + q0 * sh.ef : (uint32_t*)w->ms_lists.p;
        uint32_t* d_lcnt = a.out_list_counts ? a.out_list_counts + q0 : (uint32_t*)w->ms_lists.p + sh.chunk * (size_t)sh.ef;
        if ((rc = run_chunk(c, w, query_rows(c.ix, a.query_dim).at(a.queries, q0), n, a.out_ids + q0 * a.top_k, a.out_scores + q0 * a.top_k, a.out_counts + q0,
                            d_lists, d_lcnt, s)))
            return rc;
    }
    return RBQ_OK;
    RBQ_GUARD_END
}
} // namespace
} // namespace rbq_api

extern "C" {
// ---- MSTG posting-list scan ------------------------------------------------------------
int rbq_posting_scan_batch(const rbq_index* ch, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t top_k,
                           const uint32_t* list_ids, const uint32_t* list_counts, uint32_t max_lists,
                           uint64_t* out_ids, float* out_scores, uint32_t* out_counts) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    rbq_index* h = const_cast<rbq_index*>(ch);
    int rc = check_query_args(h, query_dim);
    if (rc) return rc;
    Replica* ix = h->reps[0];
    if (ix->rotator != RBQ_ROTATOR_NONE) return fail(RBQ_INVALID_CONFIG, "posting-list scan needs an index created with rotator NONE");
    if (nq == 0) return RBQ_OK;
    if (!queries || !list_ids || !list_counts || !out_ids || !out_scores || !out_counts) return fail(RBQ_INVALID_CONFIG, "null buffer");
    if ((rc = check_query_pointer(h, queries))) return rc;
    if (top_k == 0) { std::memset(out_counts, 0, nq * 4); return RBQ_OK; }
    if (top_k > kTopKHardMax || (uint64_t)std::min<uint64_t>(nq, 16384) * ((uint64_t)top_k + 1) * 8 > (8ull << 30))
        return fail(RBQ_INVALID_CONFIG, "top_k too large for one call (top_k <= 2^20)");
    if (max_lists == 0) { no_candidates(nq, top_k, out_ids, out_scores, out_counts); return RBQ_OK; }
    if (max_lists > (1u << 26)) return fail(RBQ_INVALID_CONFIG, "too many lists per query");
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    // exact work-list bound from the host copy of the list sizes (a list may legally repeat)
    uint64_t wl_stride = 1;
    for (uint64_t q = 0; q < nq; ++q) {
        uint64_t tot = 0;
        const uint32_t n = std::min(list_counts[q], max_lists);
        for (uint32_t r = 0; r < n; ++r) {
            const uint32_t cid = list_ids[q * max_lists + r];
            if (cid < ix->n_lists) tot += (ix->h_list_n[cid] + 31u) / 32u;
        }
        wl_stride = std::max(wl_stride, tot);
    }
    if (wl_stride > 0xffffffffull) return fail(RBQ_INVALID_CONFIG, "posting lists too long for one query");
    Workspace* w = take_ws(ix);
    if (!w) return fail(RBQ_DEVICE, "cannot create workspace stream");
    DevBuf& d_lists = w->scores; // reuse: [n][max_lists] u32
    DevBuf& d_cnts = w->nvec;    // reuse: [n] u32
    return host_chunks(ix, w, queries, nq, query_dim, top_k, 16384, out_ids, out_scores, out_counts,
                       [&](uint64_t q0, uint64_t n, const float* d_q, uint64_t* d_ids, float* d_scores, uint32_t* d_counts, hipStream_t st) -> int {
        int r2;
        if ((r2 = d_lists.ensure(n * (size_t)max_lists * 4))) return r2;
        if ((r2 = d_cnts.ensure(n * 8))) return r2;
        HIP_TRY(hipMemcpyAsync(d_lists.p, list_ids + q0 * max_lists, n * (size_t)max_lists * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_cnts.p, list_counts + q0, n * 4, hipMemcpyHostToDevice, st));
        if ((r2 = mstg_prep(ix, w, d_q, n, /*keep_ex_bits=*/false, st))) return r2;
        return scan_posting_lists(ix, w, n, (const uint32_t*)d_lists.p, (const uint32_t*)d_cnts.p, max_lists, wl_stride, top_k, d_ids, d_scores,
                                  d_counts, nullptr, st);
    });
    RBQ_GUARD_END
}

// ---- MSTG search (include/rbq_mstg.h) ------------------------------------------------------------------
int rbq_mstg_search_batch(const rbq_index* idx, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t top_k, uint32_t ef_search,
                          float pruning_epsilon, uint64_t* out_ids, float* out_scores, uint32_t* out_counts, uint32_t* out_list_ids,
                          uint32_t* out_list_counts) {
    return ms_search_host(idx, {queries, nq, query_dim, top_k, ef_search, pruning_epsilon, out_ids, out_scores, out_counts, out_list_ids, out_list_counts});
}
int rbq_mstg_search_batch_device(const rbq_index* idx, const float* d_queries, uint64_t nq, uint32_t query_dim, uint32_t top_k,
                                 uint32_t ef_search, float pruning_epsilon, uint64_t* d_out_ids, float* d_out_scores,
                                 uint32_t* d_out_counts, uint32_t* d_out_list_ids, uint32_t* d_out_list_counts, void* hip_stream) {
    return ms_search_device(idx, {d_queries, nq, query_dim, top_k, ef_search, pruning_epsilon, d_out_ids, d_out_scores, d_out_counts, d_out_list_ids,
                                  d_out_list_counts}, hip_stream);
}
int rbq_mstg_search_refined_batch(const rbq_index* idx, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t top_k,
                                  uint32_t ef_search, float pruning_epsilon, uint32_t refine_pool, uint64_t* out_ids, float* out_scores,
                                  uint32_t* out_counts, uint32_t* out_list_ids, uint32_t* out_list_counts) {
    return ms_search_host(idx, {queries, nq, query_dim, top_k, ef_search, pruning_epsilon, out_ids, out_scores, out_counts, out_list_ids, out_list_counts,
                                true, refine_pool});
}
int rbq_mstg_search_refined_batch_device(const rbq_index* idx, const float* d_queries, uint64_t nq, uint32_t query_dim, uint32_t top_k,
                                         uint32_t ef_search, float pruning_epsilon, uint32_t refine_pool, uint64_t* d_out_ids,
                                         float* d_out_scores, uint32_t* d_out_counts, uint32_t* d_out_list_ids,
                                         uint32_t* d_out_list_counts, void* hip_stream) {
    return ms_search_device(idx, {d_queries, nq, query_dim, top_k, ef_search, pruning_epsilon, d_out_ids, d_out_scores, d_out_counts, d_out_list_ids,
                                  d_out_list_counts, true, refine_pool}, hip_stream);
}

uint64_t rbq_mstg_debug_search_fallbacks(void) {
    uint64_t total = 0;
    for (int dev = 0; dev < 16; ++dev) {
        unsigned long long* p;
        { std::lock_guard<std::mutex> lk(g_ms_mu); p = g_ms_fallbacks[dev]; }
        if (!p) continue;
        DeviceGuard g(dev);
        unsigned long long v = 0;
        if (g.ok && hipMemcpy(&v, p, 8, hipMemcpyDeviceToHost) == hipSuccess) total += v;
        else (void)hipGetLastError();
    }
    return total;
}
} // extern "C"
