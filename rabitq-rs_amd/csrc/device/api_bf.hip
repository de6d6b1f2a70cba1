// api_bf.hip — brute-force index (rbq_bf_*): BruteForceRabitqIndex, reference src/brute_force.rs.
// Host side: validation, upload, training on the device (rbq_bf_train_device), RBF1 in / out, and per search call: queries -> k_prep (rotation + QueryPrecomputed constants, shared with
// the IVF path) -> for each chunk of vectors k_bf_dist + k_bf_select (bf.hpp) -> results; the range search (rbq_bf_range_batch)
// runs k_bf_range_count + k_bf_range_place (bf_range.hpp) behind k_bf_dist instead, the exact one (rbq_bf_range_exact_batch, raw rows
// attached with rbq_bf_set_rerank_vectors) k_bf_range_exact (bf_range_exact.hpp) in k_bf_range_count's place; the exact top-k
// (rbq_bf_search_exact_batch) runs the search's chain at top_k := its pool and k_bf_rerank_score + k_bf_rerank_order (bf_rerank.hpp)
// behind a sub-batch's last k_bf_select; its ranked variant (rbq_bf_search_exact_ranked_batch) forms the pool with the radix select
// of bf_pool.hpp in k_bf_select's place.  The chunks and
// sub-batches of a call are decided in csrc/host/rbq_bf_plan.hpp (plan_bf_call, pure host code); bf_run_call is the one loop that
// walks them, and the kinds of call hand it only what differs.  Each call takes a workspace and a stream of its own from the
// handle's pool, so calls on one handle may overlap.
#include <optional>

#include "bf_index.hpp"
#include "ext/rbq_bf_range.h"
#include "../host/rbq_bf_plan.hpp"

using namespace rbq_api;

namespace rbq_api {
namespace {
static_assert(rbq_host::kBfPlanLdsHeapMaxTopK == kBfLdsHeapMaxTopK && rbq_host::kBfPlanRangeSpan == kBfRangeSpan, "host plan and kernels disagree");
constexpr uint32_t kBfTopKMax = 16384;
constexpr uint64_t kBfTrainRowBudget = 512ull << 20; // rotated rows of one training pass (the IVF encoder's scratch budget)
std::atomic<uint64_t> g_bf_chunk_vectors{0};   // rbq_bf_debug_set_chunk_vectors (0: the default)
std::atomic<uint64_t> g_bf_select_launches{0}; // rbq_bf_debug_select_launches
} // namespace

void bf_free(rbq_bf_index* ix) {
    if (!ix) return;
    DeviceGuard g(ix->device);
    (void)hipDeviceSynchronize();
    for (Arr* a : {&ix->rot_blob, &ix->bin, &ix->ex}) if (a->p) (void)hipFree(a->p);
    for (Arr& a : ix->f) if (a.p) (void)hipFree(a.p);
    if (ix->raw.p && !ix->raw_borrowed) (void)hipFree(ix->raw.p);
    for (BfWorkspace* w : ix->pool) delete w;
    delete ix;
}

int bf_new_index(const rbq_header* hdr, uint64_t n, uint64_t ex_len, int dev, BfOwner& own) {
    own.ix = new rbq_bf_index();
    rbq_bf_index* ix = own.ix;
    static_cast<Geometry&>(*ix) = geometry_of(*hdr);
    ix->device = dev;
    ix->hdr = *hdr;
    ix->hdr.n_vectors = n; ix->hdr.n_lists = 0;
    ix->blob.assign(hdr->rotator_blob, hdr->rotator_blob + hdr->rotator_len);
    ix->hdr.rotator_blob = ix->blob.data();
    ix->ex_len = ex_len;
    const uint64_t D = ix->D;
    int rc;
    if ((rc = upload_arr(ix->rot_blob, ix->blob.data(), ix->blob.size())) || (rc = alloc_arr(ix->bin, n * (D / 8))) ||
        (rc = alloc_arr(ix->ex, n * (D * ix->ex_bits / 8))))
        return rc;
    for (Arr& a : ix->f) if ((rc = alloc_arr(a, n * 4))) return rc;
    return RBQ_OK;
}

int bf_encode_rows(rbq_bf_index* ix, const float* data, uint64_t n, uint64_t row0, bool opt, float t_const, uint64_t max_chunk_rows) {
    const uint32_t dim = ix->dim, D = ix->D, ex = ix->ex_bits;
    const uint64_t bin_len = D / 8, ex_bytes = (uint64_t)D * ex / 8;
    uint64_t rows = std::max<uint64_t>(64, (kBfTrainRowBudget / ((uint64_t)D * 4)) & ~63ull);
    if (max_chunk_rows) rows = std::min(rows, max_chunk_rows);
    rows = std::min(rows, n);
    const bool on_device = is_device_pointer(data);
    Scratch t;
    float *d_in = nullptr, *d_rows = nullptr, *d_zero = nullptr;
    uint8_t* d_raw = nullptr;
    double* d_t = nullptr;
    uint32_t* d_list = nullptr; // k_rescale's block -> list table: every block belongs to "list 0", the zero centroid
    if (!on_device) HIP_TRY(t.alloc(&d_in, rows * dim * 4));
    HIP_TRY(t.alloc(&d_rows, rows * D * 4));
    HIP_TRY(t.alloc(&d_raw, ex ? rows * D : 16));
    if (opt) {
        const uint64_t nb = (rows + 31) / 32;
        HIP_TRY(t.alloc(&d_t, rows * 8));
        HIP_TRY(t.alloc(&d_zero, (size_t)D * 4));
        HIP_TRY(t.alloc(&d_list, nb * 4));
        HIP_TRY(hipMemset(d_zero, 0, (size_t)D * 4));
        HIP_TRY(hipMemset(d_list, 0, nb * 4));
    }
    for (uint64_t c0 = 0; c0 < n; c0 += rows) {
        const uint32_t nr = (uint32_t)std::min<uint64_t>(rows, n - c0);
        const uint64_t r0 = row0 + c0;
        const float* src = data + c0 * dim;
        if (!on_device) {
            HIP_TRY(hipMemcpy(d_in, src, (size_t)nr * dim * 4, hipMemcpyHostToDevice));
            src = d_in;
        }
        HIP_TRY(launch_rotate_rows(src, nullptr, nr, dim, D, (int)ix->rotator, (const uint8_t*)ix->rot_blob.p, ix->trunc, ix->fac, d_rows, 0));
        if (opt) HIP_TRY(launch_rescale(d_rows, d_zero, d_list, nullptr, nullptr, nr, D, ex, false, d_t, 0));
        EncodeParams P;
        P.rows = d_rows; P.centroids = nullptr; P.slot_src = nullptr; P.block_list = nullptr; P.row_slot = nullptr; P.t_row = d_t;
        P.blocks = (uint8_t*)ix->bin.p + r0 * bin_len; P.raw_ex = d_raw; P.ids = nullptr; P.src_base = 0;
        P.delta = (float*)ix->f[0].p + r0; P.vl = (float*)ix->f[1].p + r0; P.f_add = (float*)ix->f[2].p + r0;
        P.f_rescale = (float*)ix->f[3].p + r0; P.f_error = (float*)ix->f[4].p + r0; P.residual_norm = (float*)ix->f[5].p + r0;
        P.f_add_ex = (float*)ix->f[6].p + r0; P.f_rescale_ex = (float*)ix->f[7].p + r0;
        P.nslots = nr; P.D = D; P.Dc = ix->Dc; P.ex_bits = ex; P.metric = ix->metric; P.t_const = t_const;
        HIP_TRY(launch_bf_encode(P, 0));
        if (ex) HIP_TRY(launch_bf_pack_ex(d_raw, nr, D, ex, (uint8_t*)ix->ex.p + r0 * ex_bytes, 0));
        HIP_TRY(hipDeviceSynchronize()); // the scratch (and the staging copy of a host caller's rows) is reused by the next chunk
    }
    return RBQ_OK;
}

namespace {
// The device a handle is made on (device < 0: the current one), checked against the device count; on RBQ_OK `g` has switched to it.
int bf_enter_device(int device, int* dev, std::optional<DeviceGuard>& g) {
    *dev = device;
    if (*dev < 0) HIP_TRY(hipGetDevice(dev));
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (*dev >= count) return fail(RBQ_INVALID_CONFIG, "no such device: " + std::to_string(*dev));
    g.emplace(*dev);
    if (!g->ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    return RBQ_OK;
}

// The caller's host array into an array bf_new_index has allocated (nothing to copy for an array of no bytes: n == 0, or no ex code).
int fill_arr(const Arr& a, const void* src) {
    if (a.bytes) HIP_TRY(hipMemcpy(a.p, src, a.bytes, hipMemcpyHostToDevice));
    return RBQ_OK;
}

int bf_create_impl(const rbq_header* hdr, const rbq_bf_view* v, int device, rbq_bf_index** out) {
    if (!out) return fail(RBQ_INVALID_CONFIG, "null output");
    *out = nullptr;
    int rc = validate_header(hdr, /*brute_force=*/true);
    if (rc) return rc;
    if (!v) return fail(RBQ_INVALID_CONFIG, "null view");
    const uint64_t n = v->n, D = hdr->padded_dim, ex = hdr->ex_bits;
    if (n > 0xffffffffull) return fail(RBQ_INVALID_CONFIG, "more than 2^32 vectors");
    const uint64_t ex_want = D * ex / 8;
    if (ex ? v->ex_len != ex_want : (v->ex_len != 0 && v->ex_len != D / 8)) return fail(RBQ_INVALID_CONFIG, "ex_len does not match the header");
    const float* fs[8] = {v->delta, v->vl, v->f_add, v->f_rescale, v->f_error, v->residual_norm, v->f_add_ex, v->f_rescale_ex};
    if (n) {
        if (!v->bin_codes || (ex && !v->ex_codes)) return fail(RBQ_INVALID_CONFIG, "null code array");
        for (const float* p : fs) if (!p) return fail(RBQ_INVALID_CONFIG, "null factor array");
    }
    int dev;
    std::optional<DeviceGuard> g;
    if ((rc = bf_enter_device(device, &dev, g))) return rc;
    BfOwner own{nullptr};
    if ((rc = bf_new_index(hdr, n, v->ex_len, dev, own))) return rc;
    rbq_bf_index* ix = own.ix;
    if ((rc = fill_arr(ix->bin, v->bin_codes)) || (rc = fill_arr(ix->ex, v->ex_codes))) return rc; // (ex: no bytes for a 1-bit index)
    for (int k = 0; k < 8; ++k) if ((rc = fill_arr(ix->f[k], fs[k]))) return rc;
    *out = own.release();
    return RBQ_OK;
}

// BruteForceRabitqIndex::train (src/brute_force.rs:214-285) on the device, a chunk of rows at a time: k_rotate_rows ->
// k_rescale (OPTIMAL) -> k_encode's flat mode against the zero centroid -> k_bf_pack_ex, straight into the index's arrays.
int bf_train_impl(const rbq_header* hdr, const float* data, uint64_t n, int rescale, float t_const, uint64_t max_chunk_rows, int device,
                  rbq_bf_index** out) {
    if (!out) return fail(RBQ_INVALID_CONFIG, "null output");
    *out = nullptr;
    if (!hdr) return fail(RBQ_INVALID_CONFIG, "null header");
    if (!data) return fail(RBQ_INVALID_CONFIG, "null data");
    if (n == 0) return fail(RBQ_INVALID_CONFIG, "training data must be non-empty");
    int rc = validate_header(hdr, /*brute_force=*/true);
    if (rc) return rc;
    if (n > 0xffffffffull) return fail(RBQ_INVALID_CONFIG, "more than 2^32 vectors");
    const int opt = rescale_mode(rescale, hdr);
    if (opt < 0) return RBQ_INVALID_CONFIG;
    if (!opt && hdr->ex_bits > 0 && !(t_const > 0.0f)) return fail(RBQ_INVALID_CONFIG, "the device encoder needs the constant rescale factor (faster config)");
    int dev;
    std::optional<DeviceGuard> g;
    if ((rc = bf_enter_device(device, &dev, g))) return rc;
    BfOwner own{nullptr};
    // a trained 1-bit index carries D/8 zero bytes of ex code per vector (rbq_bf_view::ex_len)
    const uint64_t D = hdr->padded_dim;
    if ((rc = bf_new_index(hdr, n, hdr->ex_bits ? D * hdr->ex_bits / 8 : D / 8, dev, own))) return rc;
    if ((rc = bf_encode_rows(own.ix, data, n, 0, opt != 0, t_const, max_chunk_rows))) return rc;
    *out = own.release();
    return RBQ_OK;
}

// ---- a search call: top-k, range and exact range ---------------------------------------------------------------------------------
// A workspace of the handle's pool for the length of one call.
struct BfLease {
    rbq_bf_index* ix;
    BfWorkspace* w = nullptr;
    explicit BfLease(rbq_bf_index* i) : ix(i) {
        {
            std::lock_guard<std::mutex> lk(ix->mu);
            if (!ix->pool.empty()) { w = ix->pool.back(); ix->pool.pop_back(); }
        }
        if (!w) w = new BfWorkspace();
    }
    ~BfLease() { std::lock_guard<std::mutex> lk(ix->mu); ix->pool.push_back(w); }
};

// The plan of a call on ix (rbq_bf_plan.hpp); `k`: top_k, or the capacity of a range call.  The test hook is read once per call.
rbq_host::BfCallPlan bf_plan(const rbq_bf_index* ix, uint64_t nq, bool range, uint32_t k) {
    rbq_host::BfCallShape s;
    s.n = ix->hdr.n_vectors; s.nq = nq; s.range = range; s.top_k = k; s.chunk_vectors = g_bf_chunk_vectors.load(std::memory_order_relaxed);
    return rbq_host::plan_bf_call(s);
}

// ONE call, as the plan cuts it: the handle's device, a workspace with its stream, the buffers of a sub-batch's prepared queries and
// their distances to a chunk, the filter; per sub-batch H2D + k_prep, per chunk k_bf_dist, then the counts back; one wait at the end.
// What the kinds of call do differently they enqueue themselves:
//   setup(w, st)                the call's own buffers, and what must be on the stream before the first query
//   chunk(w, st, m, c, v0, nv)  behind k_bf_dist of chunk c = vectors v0 .. v0 + nv - 1, for the sub-batch's m queries
//   rows(w, st, q0, m)          the rows of queries q0 .. q0 + m - 1 back to the caller
//   finish(w, st)               after the last sub-batch, before the synchronise: host work here overlaps the stream's
template <class Setup, class Chunk, class Rows, class Finish>
int bf_run_call(rbq_bf_index* ix, const rbq_host::BfCallPlan& pl, const float* queries, uint64_t nq, const uint32_t* filter_words,
                uint64_t filter_nbits, uint32_t* out_counts, Setup setup, Chunk chunk, Rows rows, Finish finish) {
    const uint64_t n = ix->hdr.n_vectors, sub = pl.sub;
    const uint32_t dim = ix->hdr.dim;
    DeviceGuard g(ix->device); // (the last check of every entry)
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    BfLease lease(ix);
    BfWorkspace* w = lease.w;
    if (!w->stream) HIP_TRY(hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking));
    hipStream_t st = w->stream;
    int rc;
    if ((rc = w->q.ensure(sub * dim * 4)) || (rc = w->rot.ensure(sub * ix->hdr.padded_dim * 4)) || (rc = w->lut.ensure(sub * 4 * ix->Dc)) ||
        (rc = w->consts.ensure(sub * sizeof(QueryConsts))) || (rc = w->dist.ensure(sub * pl.nv_chunk * 4)) || (rc = w->counts.ensure(sub * 4)))
        return rc;
    BfDistParams dp;
    dp.D = ix->hdr.padded_dim; dp.ex_bits = ix->hdr.ex_bits; dp.bin = (const uint8_t*)ix->bin.p; dp.ex = (const uint8_t*)ix->ex.p;
    dp.f_add = (const float*)ix->f[2].p; dp.f_rescale = (const float*)ix->f[3].p;
    dp.f_add_ex = (const float*)ix->f[6].p; dp.f_rescale_ex = (const float*)ix->f[7].p;
    dp.rot = (const float*)w->rot.p; dp.consts = (const QueryConsts*)w->consts.p; dp.dist = (float*)w->dist.p;
    dp.filter = nullptr; dp.filter_nbits = filter_nbits;
    if (filter_words) {
        const uint64_t words = (filter_nbits + 31) / 32;
        if ((rc = w->filter.ensure(std::max<uint64_t>(words, 1) * 4))) return rc;
        if (words) HIP_TRY(hipMemcpyAsync(w->filter.p, filter_words, words * 4, hipMemcpyHostToDevice, st));
        dp.filter = (const uint32_t*)w->filter.p;
    }
    if ((rc = setup(w, st))) return rc;
    for (uint64_t q0 = 0; q0 < nq; q0 += sub) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(sub, nq - q0);
        HIP_TRY(hipMemcpyAsync(w->q.p, queries + q0 * dim, (size_t)m * dim * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(launch_prep(prep_params(*ix, ix->rot_blob, *w, (const float*)w->q.p, m), ix->device, st));
        for (uint64_t c = 0; c < pl.n_chunks; ++c) {
            dp.nq = m; dp.v0 = c * pl.nv_chunk; dp.nv = std::min<uint64_t>(pl.nv_chunk, n - dp.v0);
            HIP_TRY(launch_bf_dist(dp, st));
            if ((rc = chunk(w, st, m, c, dp.v0, dp.nv))) return rc;
        }
        if ((rc = rows(w, st, q0, m))) return rc;
        HIP_TRY(hipMemcpyAsync(out_counts + q0, w->counts.p, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    }
    if ((rc = finish(w, st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return RBQ_OK;
}

// The select of a top-k call at K entries per query, for the two calls that run it (the search, and the exact search at K := its
// pool): the buffers of a sub-batch's heaps and K-wide rows with the heap statistics cleared, and k_bf_select behind k_bf_dist of
// chunk c, its counts going to `counts`.
int bf_select_setup(const rbq_host::BfCallPlan& pl, uint64_t K, BfWorkspace* w, hipStream_t st) {
    const uint64_t sub = pl.sub;
    int rc;
    if ((rc = w->heap_len.ensure(sub * 4)) || (rc = w->ids.ensure(sub * K * 8)) || (rc = w->scores.ensure(sub * K * 4)) || (rc = w->stats.ensure(16)))
        return rc;
    if (pl.heap_ws && ((rc = w->heap_d.ensure(sub * (K + 1) * 4)) || (rc = w->heap_s.ensure(sub * (K + 1) * 4)))) return rc;
    HIP_TRY(hipMemsetAsync(w->stats.p, 0, 16, st));
    return RBQ_OK;
}
int bf_select_chunk(const rbq_bf_index* ix, const rbq_host::BfCallPlan& pl, uint32_t K, BfWorkspace* w, hipStream_t st, uint32_t m, uint64_t c,
                    uint64_t v0, uint64_t nv, uint32_t* counts) {
    BfSelectParams sp;
    sp.dist = (const float*)w->dist.p; sp.nq = m; sp.top_k = K; sp.v0 = v0; sp.nv = nv; sp.metric = ix->hdr.metric;
    sp.first = c == 0; sp.last = c + 1 == pl.n_chunks; sp.lds_heap = pl.lds_heap;
    sp.heap_d = (float*)w->heap_d.p; sp.heap_s = (uint32_t*)w->heap_s.p; sp.heap_len = (uint32_t*)w->heap_len.p;
    sp.out_ids = (uint64_t*)w->ids.p; sp.out_scores = (float*)w->scores.p; sp.out_counts = counts;
    sp.stats = (unsigned long long*)w->stats.p;
    HIP_TRY(launch_bf_select(sp, st));
    g_bf_select_launches.fetch_add(1, std::memory_order_relaxed);
    return RBQ_OK;
}

// The rerank of a pool of K entries per query down to top_k, for the two exact top-k calls: its buffers; k_bf_rerank_score ->
// k_bf_rerank_order (bf_rerank.hpp) over the pool in w->ids / w->pool_counts of a sub-batch's m queries, which score it against the
// handle's raw rows and write the top_k-wide rows and w->counts; and the rows of a sub-batch back to the caller.
int bf_rerank_setup(uint64_t sub, uint64_t K, uint64_t top_k, BfWorkspace* w) {
    int rc;
    if ((rc = w->pool_counts.ensure(sub * 4)) || (rc = w->exact.ensure(sub * K * 4)) || (rc = w->top_ids.ensure(sub * top_k * 8)) ||
        (rc = w->top_scores.ensure(sub * top_k * 4)))
        return rc;
    return RBQ_OK;
}
int bf_rerank_pool(const rbq_bf_index* ix, uint32_t K, uint32_t top_k, BfWorkspace* w, hipStream_t st, uint32_t m) {
    uint32_t np2 = 1;
    while (np2 < K) np2 <<= 1;
    BfRerankParams rp;
    rp.queries = (const float*)w->q.p; rp.raw = ix->raw.p; rp.n_raw = ix->n_raw; rp.nq = m; rp.dim = ix->hdr.dim;
    rp.pool = K; rp.pool_np2 = np2; rp.top_k = top_k; rp.metric = ix->hdr.metric; rp.raw_dtype = ix->raw_dtype;
    rp.pool_ids = (const uint64_t*)w->ids.p; rp.pool_counts = (const uint32_t*)w->pool_counts.p; rp.exact = (float*)w->exact.p;
    rp.out_ids = (uint64_t*)w->top_ids.p; rp.out_scores = (float*)w->top_scores.p; rp.out_counts = (uint32_t*)w->counts.p;
    HIP_TRY(launch_bf_rerank_score(rp, st));
    HIP_TRY(launch_bf_rerank_order(rp, ix->device, st));
    return RBQ_OK;
}
int bf_top_k_rows(const DevBuf& ids, const DevBuf& scores, uint64_t k, hipStream_t st, uint64_t q0, uint32_t m, uint64_t* out_ids, float* out_scores) {
    HIP_TRY(hipMemcpyAsync(out_ids + q0 * k, ids.p, (size_t)m * k * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_scores + q0 * k, scores.p, (size_t)m * k * 4, hipMemcpyDeviceToHost, st));
    return RBQ_OK;
}

// exact_pool 0: rbq_bf_search_batch.  Else rbq_bf_search_exact_batch (include/ext/rbq_bf_range.h) at the pool
// P = exact_pool >= top_k: the same plan and the same select at K := P, its counts kept apart; behind the last chunk of a sub-batch
// k_bf_rerank_score -> k_bf_rerank_order (bf_rerank.hpp) score the pool against the handle's raw rows and write the top_k-wide rows
// and the counts, which go back in the select's rows' place.
int bf_search_impl(rbq_bf_index* ix, const float* queries, uint64_t nq, uint32_t top_k, uint32_t exact_pool, const uint32_t* filter_words,
                   uint64_t filter_nbits, uint64_t* out_ids, float* out_scores, uint32_t* out_counts) {
    const uint32_t K = exact_pool ? exact_pool : top_k;
    const rbq_host::BfCallPlan pl = bf_plan(ix, nq, /*range=*/false, K);
    const uint64_t sub = pl.sub, k = top_k;
    uint64_t stats[2] = {0, 0};
    const int rc = bf_run_call(
        ix, pl, queries, nq, filter_words, filter_nbits, out_counts,
        [&](BfWorkspace* w, hipStream_t st) -> int {
            int rc;
            if (exact_pool && (rc = bf_rerank_setup(sub, K, k, w))) return rc;
            return bf_select_setup(pl, K, w, st);
        },
        [&](BfWorkspace* w, hipStream_t st, uint32_t m, uint64_t c, uint64_t v0, uint64_t nv) -> int {
            int rc;
            if ((rc = bf_select_chunk(ix, pl, K, w, st, m, c, v0, nv, (uint32_t*)(exact_pool ? w->pool_counts.p : w->counts.p)))) return rc;
            if (!exact_pool || c + 1 != pl.n_chunks) return RBQ_OK;
            return bf_rerank_pool(ix, K, top_k, w, st, m);
        },
        [&](BfWorkspace* w, hipStream_t st, uint64_t q0, uint32_t m) -> int {
            return bf_top_k_rows(exact_pool ? w->top_ids : w->ids, exact_pool ? w->top_scores : w->scores, k, st, q0, m, out_ids, out_scores);
        },
        [&](BfWorkspace* w, hipStream_t st) -> int {
            HIP_TRY(hipMemcpyAsync(stats, w->stats.p, 16, hipMemcpyDeviceToHost, st));
            return RBQ_OK;
        });
    if (rc == RBQ_OK) { ix->pushes += stats[0]; ix->tie_pushes += stats[1]; }
    return rc;
}

// rbq_bf_search_exact_ranked_batch (include/ext/rbq_bf_range.h): the exact search with the pool chosen by rank
// — the P best estimates by (total_cmp order, id) — and no heap.  The range search's plan at capacity P gives the spans of a chunk
// and a sub-batch within the output budget; per chunk launch_bf_pool_rank (bf_pool.hpp) behind k_bf_dist, the pool so far carried
// from chunk to chunk in two lists that alternate (w->carry, their lengths in w->running); behind the last chunk the rerank above.
int bf_search_ranked_impl(rbq_bf_index* ix, const float* queries, uint64_t nq, uint32_t top_k, uint32_t P, const uint32_t* filter_words,
                          uint64_t filter_nbits, uint64_t* out_ids, float* out_scores, uint32_t* out_counts) {
    const rbq_host::BfCallPlan pl = bf_plan(ix, nq, /*range=*/true, P);
    const uint64_t sub = pl.sub, k = top_k;
    const uint32_t carry_blocks = (P + kBfRangeSpan - 1) / kBfRangeSpan;
    return bf_run_call(
        ix, pl, queries, nq, filter_words, filter_nbits, out_counts,
        [&](BfWorkspace* w, hipStream_t) -> int {
            int rc;
            if ((rc = bf_rerank_setup(sub, P, k, w)) || (rc = w->ids.ensure(sub * P * 8)) || (rc = w->pool_hist.ensure(sub * kBfPoolPasses * kBfPoolBins * 4)) ||
                (rc = w->pool_state.ensure(sub * (kBfPoolPasses + 1) * 8)) || (rc = w->span_counts.ensure(2 * sub * (pl.spans + carry_blocks) * 4)))
                return rc;
            if (pl.n_chunks > 1 && ((rc = w->carry.ensure(2 * sub * P * 8)) || (rc = w->running.ensure(2 * sub * 4)))) return rc;
            return RBQ_OK;
        },
        [&](BfWorkspace* w, hipStream_t st, uint32_t m, uint64_t c, uint64_t v0, uint64_t nv) -> int {
            BfPoolParams pp;
            pp.dist = (const float*)w->dist.p; pp.nq = m; pp.n_spans = (uint32_t)((nv + kBfRangeSpan - 1) / kBfRangeSpan);
            pp.first = c == 0; pp.last = c + 1 == pl.n_chunks; pp.n_carry = pp.first ? 0u : carry_blocks;
            pp.v0 = v0; pp.nv = nv; pp.pool = P;
            pp.hist = (uint32_t*)w->pool_hist.p; pp.state = (uint32_t*)w->pool_state.p; pp.span_counts = (uint32_t*)w->span_counts.p;
            unsigned long long* lists = (unsigned long long*)w->carry.p; // (null with one chunk: neither side is then used)
            uint32_t* lens = (uint32_t*)w->running.p;
            pp.carry_in = pp.first ? nullptr : lists + (c & 1) * sub * P; pp.carry_n_in = pp.first ? nullptr : lens + (c & 1) * sub;
            pp.carry_out = pp.last ? nullptr : lists + ((c + 1) & 1) * sub * P; pp.carry_n_out = pp.last ? nullptr : lens + ((c + 1) & 1) * sub;
            pp.out_ids = (uint64_t*)w->ids.p; pp.out_counts = (uint32_t*)w->pool_counts.p;
            HIP_TRY(launch_bf_pool_rank(pp, st));
            return pp.last ? bf_rerank_pool(ix, P, top_k, w, st, m) : RBQ_OK;
        },
        [&](BfWorkspace* w, hipStream_t st, uint64_t q0, uint32_t m) -> int { return bf_top_k_rows(w->top_ids, w->top_scores, k, st, q0, m, out_ids, out_scores); },
        [&](BfWorkspace*, hipStream_t) -> int { return RBQ_OK; });
}

// rbq_bf_range_batch (include/ext/rbq_bf_range.h): the search's plan without its heap — per chunk of vectors
// k_bf_range_count -> k_bf_range_place (bf_range.hpp) behind k_bf_dist, the totals carried from chunk to chunk in two arrays that
// alternate.  The sub-batch comes from the distance budget and, with rows, the output budget.
// exact_x (rbq_bf_range_exact_batch; null: the estimate decides): `radius` is the candidate radius,
// k_bf_range_exact (bf_range_exact.hpp) stands in k_bf_range_count's place — it scores the candidates against the handle's raw rows
// and writes the exact distances over the workspace — and k_bf_range_place runs at the radius *exact_x.  Everything else is one copy.
int bf_range_impl(rbq_bf_index* ix, const float* queries, uint64_t nq, uint32_t capacity, float radius, const float* exact_x,
                  const uint32_t* filter_words, uint64_t filter_nbits, uint64_t* out_ids, float* out_scores, uint32_t* out_counts) {
    const rbq_host::BfCallPlan pl = bf_plan(ix, nq, /*range=*/true, capacity);
    const uint64_t cap = pl.cap, sub = pl.sub;
    return bf_run_call(
        ix, pl, queries, nq, filter_words, filter_nbits, out_counts,
        [&](BfWorkspace* w, hipStream_t) -> int {
            int rc;
            if ((rc = w->span_counts.ensure(sub * pl.spans * 4)) || (rc = w->running.ensure(2 * sub * 4))) return rc;
            if (cap && ((rc = w->ids.ensure(sub * cap * 8)) || (rc = w->scores.ensure(sub * cap * 4)))) return rc;
            return RBQ_OK;
        },
        [&](BfWorkspace* w, hipStream_t st, uint32_t m, uint64_t c, uint64_t v0, uint64_t nv) -> int {
            BfRangeParams rp;
            rp.dist = (const float*)w->dist.p; rp.nq = m; rp.n_spans = (uint32_t)((nv + kBfRangeSpan - 1) / kBfRangeSpan);
            rp.v0 = v0; rp.nv = nv; rp.radius = exact_x ? *exact_x : radius; rp.metric = ix->hdr.metric; rp.first = c == 0; rp.last = c + 1 == pl.n_chunks;
            rp.capacity = (uint32_t)cap; rp.span_counts = (uint32_t*)w->span_counts.p;
            rp.run_in = (const uint32_t*)w->running.p + (c & 1) * sub; rp.run_out = (uint32_t*)w->running.p + ((c + 1) & 1) * sub;
            rp.out_ids = (uint64_t*)w->ids.p; rp.out_scores = (float*)w->scores.p; rp.out_counts = (uint32_t*)w->counts.p;
            if (exact_x) {
                BfRangeExactParams xp;
                xp.dist = (float*)w->dist.p; xp.queries = (const float*)w->q.p; xp.raw = ix->raw.p; xp.nq = m; xp.n_spans = rp.n_spans;
                xp.dim = ix->hdr.dim; xp.v0 = v0; xp.nv = nv; xp.candidate_radius = radius; xp.x = *exact_x; xp.metric = ix->hdr.metric;
                xp.raw_dtype = ix->raw_dtype; xp.span_counts = rp.span_counts;
                HIP_TRY(launch_bf_range_exact(xp, st));
            } else {
                HIP_TRY(launch_bf_range_count(rp, st));
            }
            HIP_TRY(launch_bf_range_place(rp, st));
            return RBQ_OK;
        },
        [&](BfWorkspace* w, hipStream_t st, uint64_t q0, uint32_t m) -> int {
            if (cap == capacity && cap) {
                HIP_TRY(hipMemcpyAsync(out_ids + q0 * cap, w->ids.p, (size_t)m * cap * 8, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipMemcpyAsync(out_scores + q0 * cap, w->scores.p, (size_t)m * cap * 4, hipMemcpyDeviceToHost, st));
            } else if (cap) { // capacity > n: the caller's rows are wider than the device's
                HIP_TRY(hipMemcpy2DAsync(out_ids + q0 * capacity, (size_t)capacity * 8, w->ids.p, cap * 8, cap * 8, m, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipMemcpy2DAsync(out_scores + q0 * capacity, (size_t)capacity * 4, w->scores.p, cap * 4, cap * 4, m, hipMemcpyDeviceToHost, st));
            }
            return RBQ_OK;
        },
        [&](BfWorkspace*, hipStream_t) -> int {
            // capacity > n: slots n .. capacity - 1 of a row can hold no match whatever the device finds; they are written here, beside
            // the copies above, while the stream works
            for (uint64_t q = 0; cap < capacity && q < nq; ++q) {
                std::fill_n(out_ids + q * capacity + cap, capacity - cap, ~0ull);
                std::fill_n(out_scores + q * capacity + cap, capacity - cap, std::numeric_limits<float>::quiet_NaN());
            }
            return RBQ_OK;
        });
}
} // namespace
} // namespace rbq_api

extern "C" {
int rbq_bf_create(const rbq_header* hdr, const rbq_bf_view* view, int device, rbq_bf_index** out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return bf_create_impl(hdr, view, device, out);
    RBQ_GUARD_END
}

int rbq_bf_train_device(const rbq_header* hdr, const float* data, uint64_t n, int rescale, float t_const, uint64_t max_chunk_rows,
                        int device, rbq_bf_index** out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return bf_train_impl(hdr, data, n, rescale, t_const, max_chunk_rows, device, out);
    RBQ_GUARD_END
}

int rbq_bf_load_rbf1(const void* bytes, size_t len, int device, rbq_bf_index** out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    if (!out) return fail(RBQ_INVALID_CONFIG, "null output");
    *out = nullptr;
    rbq_header h;
    rbq_host::BfSrc b;
    std::string detail;
    int rc = rbq_host::rbf1_parse(bytes, len, &h, &b, &detail);
    if (rc) return fail(rc, detail);
    rc = validate_header(&h, /*brute_force=*/true); // what this build cannot serve (ex_bits outside {0,2,6}, padded_dim > 2048 ...)
    if (rc) return rc;
    if (b.bin_len != h.padded_dim / 8 || b.ex_len != (size_t)h.padded_dim * h.ex_bits / 8) return fail(RBQ_INVALID_CONFIG, "unsupported code layout");
    std::vector<uint8_t> bin(b.n * b.bin_len), ex(b.n * b.ex_len);
    std::vector<float> f[8];
    for (auto& a : f) a.resize(b.n);
    for (uint64_t v = 0; v < b.n; ++v) {
        const uint8_t* r = b.rec0 + v * b.stride;
        std::memcpy(bin.data() + v * b.bin_len, r, b.bin_len);
        if (b.ex_len) std::memcpy(ex.data() + v * b.ex_len, r + b.bin_len, b.ex_len);
        for (int k = 0; k < 8; ++k) std::memcpy(&f[k][v], r + b.bin_len + b.ex_len + 4 * k, 4);
    }
    rbq_bf_view view;
    view.n = b.n; view.bin_codes = bin.data(); view.ex_codes = ex.empty() ? nullptr : ex.data(); view.ex_len = b.ex_len;
    view.delta = f[0].data(); view.vl = f[1].data(); view.f_add = f[2].data(); view.f_rescale = f[3].data();
    view.f_error = f[4].data(); view.residual_norm = f[5].data(); view.f_add_ex = f[6].data(); view.f_rescale_ex = f[7].data();
    return bf_create_impl(&h, &view, device, out);
    RBQ_GUARD_END
}

int rbq_bf_save_rbf1(const rbq_bf_index* ch, uint8_t** bytes, uint64_t* len) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    if (!ch) return fail(RBQ_INVALID_CONFIG, "null index");
    if (!bytes || !len) return fail(RBQ_INVALID_CONFIG, "null output");
    rbq_bf_index* ix = const_cast<rbq_bf_index*>(ch);
    const uint64_t n = ix->hdr.n_vectors, D = ix->hdr.padded_dim, exb = D * ix->hdr.ex_bits / 8;
    std::vector<uint8_t> bin(n * (D / 8)), ex(n * exb);
    std::vector<float> f[8];
    {
        DeviceGuard g(ix->device);
        if (n) HIP_TRY(hipMemcpy(bin.data(), ix->bin.p, bin.size(), hipMemcpyDeviceToHost));
        if (!ex.empty()) HIP_TRY(hipMemcpy(ex.data(), ix->ex.p, ex.size(), hipMemcpyDeviceToHost));
        for (int k = 0; k < 8; ++k) {
            f[k].resize(n);
            if (n) HIP_TRY(hipMemcpy(f[k].data(), ix->f[k].p, n * 4, hipMemcpyDeviceToHost));
        }
    }
    const float* fp[8];
    for (int k = 0; k < 8; ++k) fp[k] = f[k].data();
    // ex_bits == 0: the ex_len zero bytes per vector of a trained index (null source = zeros)
    const std::vector<uint8_t> o = rbq_host::rbf1_write(ix->hdr, n, bin.data(), exb ? ex.data() : nullptr, ix->ex_len, fp);
    uint8_t* p = (uint8_t*)std::malloc(o.size());
    if (!p) return fail(RBQ_IO, "out of host memory");
    std::memcpy(p, o.data(), o.size());
    *bytes = p;
    *len = o.size();
    return RBQ_OK;
    RBQ_GUARD_END
}

void rbq_bf_free_bytes(uint8_t* p) { std::free(p); }
void rbq_bf_destroy(rbq_bf_index* idx) { bf_free(idx); }
uint64_t rbq_bf_len(const rbq_bf_index* idx) { return idx ? idx->hdr.n_vectors : 0; }
uint32_t rbq_bf_dim(const rbq_bf_index* idx) { return idx ? idx->hdr.dim : 0; }
uint32_t rbq_bf_padded_dim(const rbq_bf_index* idx) { return idx ? idx->hdr.padded_dim : 0; }
uint32_t rbq_bf_metric(const rbq_bf_index* idx) { return idx ? idx->hdr.metric : RBQ_METRIC_L2; }

void rbq_bf_debug_heap_stats(const rbq_bf_index* idx, uint64_t* out2) {
    if (!idx || !out2) return;
    out2[0] = idx->pushes.load();
    out2[1] = idx->tie_pushes.load();
}
uint64_t rbq_bf_debug_set_chunk_vectors(uint64_t vectors) { return g_bf_chunk_vectors.exchange(vectors, std::memory_order_relaxed); }
uint64_t rbq_bf_debug_select_launches(void) { return g_bf_select_launches.load(std::memory_order_relaxed); }

// The checks of the search entries, in the order callers see them:
//   rbq_bf_search_batch:   null index, empty index, dimension, nq == 0 (OK) | top_k == 0 (counts zeroed, OK), top_k > 16384 |
//                          nq >= 2^31 | null buffer | the device
//   rbq_bf_search_exact_batch, rbq_bf_search_exact_ranked_batch: null index, empty index, dimension, nq == 0 (OK) | top_k == 0 (counts zeroed, OK), raw vectors
//                          attached, max(pool, top_k) > 4096 | nq >= 2^31 | null buffer | the device
//   the two range entries: null index, empty index, dimension, nq == 0 (OK) | raw vectors attached (exact) |
//                          nq >= 2^31 | null buffer, x is NaN, radius is NaN | the device
// bf_entry_prefix is the first group of either, and bf_run_call switches to the device before anything else, which is the last;
// what stands between differs and stays with its entry.  *ix null: the call is answered and the return value is its result.
static int bf_entry_prefix(const rbq_bf_index* ch, uint32_t query_dim, uint64_t nq, rbq_bf_index** ix) {
    *ix = nullptr;
    if (!ch) return fail(RBQ_INVALID_CONFIG, "null index");
    if (ch->hdr.n_vectors == 0) return fail(RBQ_EMPTY_INDEX, "index is empty");
    if (query_dim != ch->hdr.dim) {
        char b[96];
        std::snprintf(b, sizeof b, "expected %u, got %u", ch->hdr.dim, query_dim);
        return fail(RBQ_DIMENSION_MISMATCH, b);
    }
    if (nq) *ix = const_cast<rbq_bf_index*>(ch);
    return RBQ_OK;
}

int rbq_bf_search_batch(const rbq_bf_index* ch, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t top_k,
                        const uint32_t* filter_words, uint64_t filter_nbits, uint64_t* out_ids, float* out_scores, uint32_t* out_counts) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    rbq_bf_index* ix;
    const int rc = bf_entry_prefix(ch, query_dim, nq, &ix);
    if (!ix) return rc;
    if (top_k == 0) {
        if (out_counts) std::memset(out_counts, 0, nq * 4);
        return RBQ_OK;
    }
    if (top_k > kBfTopKMax) return fail(RBQ_INVALID_CONFIG, "top_k > 16384 is not supported by the brute-force index");
    if (nq >= (1ull << 31)) return fail(RBQ_INVALID_CONFIG, "nq >= 2^31");
    if (!queries || !out_ids || !out_scores || !out_counts) return fail(RBQ_INVALID_CONFIG, "null buffer");
    return bf_search_impl(ix, queries, nq, top_k, /*exact_pool=*/0, filter_words, filter_nbits, out_ids, out_scores, out_counts);
    RBQ_GUARD_END
}

// The checks of the two exact top-k entries, in their order, then the call.  ranked: rbq_bf_search_exact_ranked_batch.
static int bf_exact_entry(const rbq_bf_index* ch, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t top_k, uint32_t pool, bool ranked,
                          const uint32_t* filter_words, uint64_t filter_nbits, uint64_t* out_ids, float* out_scores, uint32_t* out_counts) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    rbq_bf_index* ix;
    const int rc = bf_entry_prefix(ch, query_dim, nq, &ix);
    if (!ix) return rc;
    if (top_k == 0) {
        if (out_counts) std::memset(out_counts, 0, nq * 4);
        return RBQ_OK;
    }
    if (!ix->raw.p) return fail(RBQ_INVALID_CONFIG, "exact search needs raw vectors attached (rbq_bf_set_rerank_vectors)");
    const uint32_t P = std::max(pool, top_k);
    if (P > kBfRerankPoolMax) return fail(RBQ_INVALID_CONFIG, "max(pool, top_k) > 4096 is not supported by the exact brute-force search");
    if (nq >= (1ull << 31)) return fail(RBQ_INVALID_CONFIG, "nq >= 2^31");
    if (!queries || !out_ids || !out_scores || !out_counts) return fail(RBQ_INVALID_CONFIG, "null buffer");
    if (ranked) return bf_search_ranked_impl(ix, queries, nq, top_k, P, filter_words, filter_nbits, out_ids, out_scores, out_counts);
    return bf_search_impl(ix, queries, nq, top_k, P, filter_words, filter_nbits, out_ids, out_scores, out_counts);
    RBQ_GUARD_END
}

int rbq_bf_search_exact_batch(const rbq_bf_index* ch, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t top_k, uint32_t pool,
                              const uint32_t* filter_words, uint64_t filter_nbits, uint64_t* out_ids, float* out_scores,
                              uint32_t* out_counts) {
    return bf_exact_entry(ch, queries, nq, query_dim, top_k, pool, /*ranked=*/false, filter_words, filter_nbits, out_ids, out_scores, out_counts);
}

int rbq_bf_search_exact_ranked_batch(const rbq_bf_index* ch, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t top_k, uint32_t pool,
                                     const uint32_t* filter_words, uint64_t filter_nbits, uint64_t* out_ids, float* out_scores,
                                     uint32_t* out_counts) {
    return bf_exact_entry(ch, queries, nq, query_dim, top_k, pool, /*ranked=*/true, filter_words, filter_nbits, out_ids, out_scores, out_counts);
}

// The checks of the two range entries, in their order, then the call.  exact_x null: rbq_bf_range_batch at `radius`; else
// rbq_bf_range_exact_batch with `radius` its candidate radius.
static int bf_range_entry(const rbq_bf_index* ch, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t capacity, float radius,
                          const float* exact_x, const uint32_t* filter_words, uint64_t filter_nbits, uint64_t* out_ids, float* out_scores,
                          uint32_t* out_counts) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    rbq_bf_index* ix;
    const int rc = bf_entry_prefix(ch, query_dim, nq, &ix);
    if (!ix) return rc;
    if (exact_x && !ix->raw.p) return fail(RBQ_INVALID_CONFIG, "exact range search needs raw vectors attached (rbq_bf_set_rerank_vectors)");
    if (nq >= (1ull << 31)) return fail(RBQ_INVALID_CONFIG, "nq >= 2^31");
    if (!queries || !out_counts || (capacity && (!out_ids || !out_scores))) return fail(RBQ_INVALID_CONFIG, "null buffer");
    if (exact_x && *exact_x != *exact_x) return fail(RBQ_INVALID_CONFIG, "x is NaN");
    if (radius != radius) return fail(RBQ_INVALID_CONFIG, exact_x ? "candidate_radius is NaN" : "radius is NaN");
    return bf_range_impl(ix, queries, nq, capacity, radius, exact_x, filter_words, filter_nbits, out_ids, out_scores, out_counts);
    RBQ_GUARD_END
}

int rbq_bf_range_batch(const rbq_bf_index* ch, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t capacity, float radius,
                       const uint32_t* filter_words, uint64_t filter_nbits, uint64_t* out_ids, float* out_scores, uint32_t* out_counts) {
    return bf_range_entry(ch, queries, nq, query_dim, capacity, radius, nullptr, filter_words, filter_nbits, out_ids, out_scores, out_counts);
}

int rbq_bf_range_exact_batch(const rbq_bf_index* ch, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t capacity, float x,
                             float candidate_radius, const uint32_t* filter_words, uint64_t filter_nbits, uint64_t* out_ids,
                             float* out_scores, uint32_t* out_counts) {
    return bf_range_entry(ch, queries, nq, query_dim, capacity, candidate_radius, &x, filter_words, filter_nbits, out_ids, out_scores,
                          out_counts);
}

// Raw rows for the exact range search.  n and the dtype are checked before the first HIP call; the alignment
// of a borrowed 16-bit pointer as soon as the memory is known to be the device's.  The new copy exists before the old rows go, so a
// failure leaves the handle as it was.
int rbq_bf_set_rerank_vectors(rbq_bf_index* ix, const void* vectors, uint64_t n, int raw_dtype) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    if (!ix) return fail(RBQ_INVALID_CONFIG, "null index");
    const bool attach = vectors != nullptr;
    if (attach) {
        if (raw_dtype != RBQ_RAW_F32 && raw_dtype != RBQ_RAW_F16 && raw_dtype != RBQ_RAW_BF16)
            return fail(RBQ_INVALID_CONFIG, "rerank vectors: unknown raw dtype " + std::to_string(raw_dtype));
        if (n != ix->hdr.n_vectors)
            return fail(RBQ_INVALID_CONFIG, "rerank vectors: " + std::to_string(n) + " rows for an index of " + std::to_string(ix->hdr.n_vectors) +
                                                " vectors (ids are positions)");
    }
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    RawRows fresh;
    if (attach && n) {
        const RawSource src(vectors);
        // (borrowed rows stay the caller's and must outlive the attachment)
        if (src.on_dev && src.device == ix->device && raw_dtype != RBQ_RAW_F32 && (reinterpret_cast<uintptr_t>(vectors) & 1u))
            return fail(RBQ_INVALID_CONFIG, "rerank vectors: a device pointer to 16-bit rows must be 2-byte aligned");
        const int rc = raw_rows_on(ix->device, src, (size_t)n * ix->hdr.dim * raw_elem_bytes(raw_dtype), fresh);
        if (rc) return rc;
    }
    const hipError_t e = hipDeviceSynchronize(); // (the old rows go: not safe concurrently with calls on the handle)
    if (e != hipSuccess) {
        raw_rows_drop(fresh);
        return fail(RBQ_DEVICE, std::string("hipDeviceSynchronize: ") + hipGetErrorString(e));
    }
    raw_rows_swap(ix, fresh, n, raw_dtype);
    return RBQ_OK;
    RBQ_GUARD_END
}

int rbq_bf_rerank_dtype(const rbq_bf_index* idx) { return idx && idx->raw.p ? idx->raw_dtype : -1; }
} // extern "C"
