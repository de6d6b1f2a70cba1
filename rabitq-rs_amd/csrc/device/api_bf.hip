// api_bf.hip — brute-force index (rbq_bf_*): BruteForceRabitqIndex, reference src/brute_force.rs.
// Host side: validation, upload, training on the device (rbq_bf_train_device), RBF1 in / out, and per search call: queries -> k_prep (rotation + QueryPrecomputed constants, shared with
// the IVF path) -> for each chunk of vectors k_bf_dist + k_bf_select (bf.hpp) -> results.  Each call takes a workspace and a stream
// of its own from the handle's pool, so calls on one handle may overlap.
#include "bf_index.hpp"

using namespace rbq_api;

namespace rbq_api {
namespace {
constexpr uint32_t kBfTopKMax = 16384;
constexpr uint64_t kBfDistBudget = 128ull << 20; // distance workspace of one sub-batch (bytes)
constexpr uint64_t kBfHeapBudget = 48ull << 20;  // heap workspace (between vector chunks, or for top_k above the LDS heap)
constexpr uint64_t kBfOutBudget = 48ull << 20;   // result buffers of one sub-batch
constexpr uint64_t kBfMaxSubBatch = 1024;
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
    int dev = device;
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (dev >= count) return fail(RBQ_INVALID_CONFIG, "no such device: " + std::to_string(dev));
    std::unique_ptr<rbq_bf_index> ix(new rbq_bf_index());
    static_cast<Geometry&>(*ix) = geometry_of(*hdr);
    ix->device = dev;
    ix->hdr = *hdr;
    ix->hdr.n_vectors = n; ix->hdr.n_lists = 0;
    ix->blob.assign(hdr->rotator_blob, hdr->rotator_blob + hdr->rotator_len);
    ix->hdr.rotator_blob = ix->blob.data();
    ix->ex_len = v->ex_len;
    DeviceGuard g(dev);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    rc = upload_arr(ix->rot_blob, ix->blob.data(), ix->blob.size());
    if (!rc) rc = upload_arr(ix->bin, v->bin_codes, n * (D / 8));
    if (!rc) rc = ex ? upload_arr(ix->ex, v->ex_codes, n * ex_want) : alloc_arr(ix->ex, 0);
    for (int k = 0; k < 8 && !rc; ++k) rc = upload_arr(ix->f[k], fs[k], n * 4);
    if (rc) { bf_free(ix.release()); return rc; }
    *out = ix.release();
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
    int dev = device;
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (dev >= count) return fail(RBQ_INVALID_CONFIG, "no such device: " + std::to_string(dev));
    DeviceGuard g(dev);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");

    BfOwner own{nullptr};
    // a trained 1-bit index carries D/8 zero bytes of ex code per vector (rbq_bf_view::ex_len)
    const uint64_t D = hdr->padded_dim;
    if ((rc = bf_new_index(hdr, n, hdr->ex_bits ? D * hdr->ex_bits / 8 : D / 8, dev, own))) return rc;
    if ((rc = bf_encode_rows(own.ix, data, n, 0, opt != 0, t_const, max_chunk_rows))) return rc;
    *out = own.release();
    return RBQ_OK;
}

int bf_search_impl(rbq_bf_index* ix, const float* queries, uint64_t nq, uint32_t top_k, const uint32_t* filter_words, uint64_t filter_nbits,
                   uint64_t* out_ids, float* out_scores, uint32_t* out_counts) {
    const uint64_t n = ix->hdr.n_vectors, K = top_k;
    const uint32_t dim = ix->hdr.dim, D = ix->hdr.padded_dim;
    // plan: vector chunks of at most kBfDistBudget / 4 vectors, sub-batches of queries within the workspace budgets
    const uint64_t cap = g_bf_chunk_vectors.load(std::memory_order_relaxed); // (test hook: read once per call)
    const uint64_t nv_chunk = std::min<uint64_t>({n, kBfDistBudget / 4, cap ? cap : UINT64_MAX});
    const uint64_t n_chunks = (n + nv_chunk - 1) / nv_chunk;
    const bool lds_heap = top_k <= kBfLdsHeapMaxTopK;
    const bool heap_ws = n_chunks > 1 || !lds_heap;
    uint64_t sub = std::min<uint64_t>({nq, kBfMaxSubBatch, std::max<uint64_t>(1, kBfDistBudget / (nv_chunk * 4)),
                                       std::max<uint64_t>(1, kBfOutBudget / (K * 12))});
    if (heap_ws) sub = std::min<uint64_t>(sub, std::max<uint64_t>(1, kBfHeapBudget / ((K + 1) * 8)));
    BfWorkspace* w = nullptr;
    {
        std::lock_guard<std::mutex> lk(ix->mu);
        if (!ix->pool.empty()) { w = ix->pool.back(); ix->pool.pop_back(); }
    }
    if (!w) w = new BfWorkspace();
    struct Give { rbq_bf_index* ix; BfWorkspace* w; ~Give() { std::lock_guard<std::mutex> lk(ix->mu); ix->pool.push_back(w); } } give{ix, w};
    if (!w->stream) HIP_TRY(hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking));
    hipStream_t st = w->stream;
    int rc;
    if ((rc = w->q.ensure(sub * dim * 4)) || (rc = w->rot.ensure(sub * D * 4)) || (rc = w->lut.ensure(sub * 4 * ix->Dc)) ||
        (rc = w->consts.ensure(sub * sizeof(QueryConsts))) || (rc = w->dist.ensure(sub * nv_chunk * 4)) ||
        (rc = w->heap_len.ensure(sub * 4)) || (rc = w->ids.ensure(sub * K * 8)) || (rc = w->scores.ensure(sub * K * 4)) ||
        (rc = w->counts.ensure(sub * 4)) || (rc = w->stats.ensure(16)))
        return rc;
    if (heap_ws && ((rc = w->heap_d.ensure(sub * (K + 1) * 4)) || (rc = w->heap_s.ensure(sub * (K + 1) * 4)))) return rc;
    const uint32_t* d_filter = nullptr;
    if (filter_words) {
        const uint64_t words = (filter_nbits + 31) / 32;
        if ((rc = w->filter.ensure(std::max<uint64_t>(words, 1) * 4))) return rc;
        if (words) HIP_TRY(hipMemcpyAsync(w->filter.p, filter_words, words * 4, hipMemcpyHostToDevice, st));
        d_filter = (const uint32_t*)w->filter.p;
    }
    HIP_TRY(hipMemsetAsync(w->stats.p, 0, 16, st));
    for (uint64_t q0 = 0; q0 < nq; q0 += sub) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(sub, nq - q0);
        HIP_TRY(hipMemcpyAsync(w->q.p, queries + q0 * dim, (size_t)m * dim * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(launch_prep(prep_params(*ix, ix->rot_blob, *w, (const float*)w->q.p, m), ix->device, st));
        for (uint64_t c = 0; c < n_chunks; ++c) {
            const uint64_t v0 = c * nv_chunk, nv = std::min<uint64_t>(nv_chunk, n - v0);
            BfDistParams dp;
            dp.rot = (const float*)w->rot.p; dp.consts = (const QueryConsts*)w->consts.p; dp.nq = m; dp.D = D; dp.ex_bits = ix->hdr.ex_bits;
            dp.v0 = v0; dp.nv = nv; dp.bin = (const uint8_t*)ix->bin.p; dp.ex = (const uint8_t*)ix->ex.p;
            dp.f_add = (const float*)ix->f[2].p; dp.f_rescale = (const float*)ix->f[3].p;
            dp.f_add_ex = (const float*)ix->f[6].p; dp.f_rescale_ex = (const float*)ix->f[7].p;
            dp.filter = d_filter; dp.filter_nbits = filter_nbits; dp.dist = (float*)w->dist.p;
            HIP_TRY(launch_bf_dist(dp, st));
            BfSelectParams sp;
            sp.dist = (const float*)w->dist.p; sp.nq = m; sp.top_k = top_k; sp.v0 = v0; sp.nv = nv; sp.metric = ix->hdr.metric;
            sp.first = c == 0; sp.last = c + 1 == n_chunks; sp.lds_heap = lds_heap;
            sp.heap_d = (float*)w->heap_d.p; sp.heap_s = (uint32_t*)w->heap_s.p; sp.heap_len = (uint32_t*)w->heap_len.p;
            sp.out_ids = (uint64_t*)w->ids.p; sp.out_scores = (float*)w->scores.p; sp.out_counts = (uint32_t*)w->counts.p;
            sp.stats = (unsigned long long*)w->stats.p;
            HIP_TRY(launch_bf_select(sp, st));
            g_bf_select_launches.fetch_add(1, std::memory_order_relaxed);
        }
        HIP_TRY(hipMemcpyAsync(out_ids + q0 * K, w->ids.p, (size_t)m * K * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_scores + q0 * K, w->scores.p, (size_t)m * K * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_counts + q0, w->counts.p, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    }
    uint64_t stats[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(stats, w->stats.p, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    ix->pushes += stats[0];
    ix->tie_pushes += stats[1];
    return RBQ_OK;
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

void rbq_bf_debug_heap_stats(const rbq_bf_index* idx, uint64_t* out2) {
    if (!idx || !out2) return;
    out2[0] = idx->pushes.load();
    out2[1] = idx->tie_pushes.load();
}
uint64_t rbq_bf_debug_set_chunk_vectors(uint64_t vectors) { return g_bf_chunk_vectors.exchange(vectors, std::memory_order_relaxed); }
uint64_t rbq_bf_debug_select_launches(void) { return g_bf_select_launches.load(std::memory_order_relaxed); }

int rbq_bf_search_batch(const rbq_bf_index* ch, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t top_k,
                        const uint32_t* filter_words, uint64_t filter_nbits, uint64_t* out_ids, float* out_scores, uint32_t* out_counts) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    if (!ch) return fail(RBQ_INVALID_CONFIG, "null index");
    rbq_bf_index* ix = const_cast<rbq_bf_index*>(ch);
    if (ix->hdr.n_vectors == 0) return fail(RBQ_EMPTY_INDEX, "index is empty");
    if (query_dim != ix->hdr.dim) {
        char b[96];
        std::snprintf(b, sizeof b, "expected %u, got %u", ix->hdr.dim, query_dim);
        return fail(RBQ_DIMENSION_MISMATCH, b);
    }
    if (nq == 0) return RBQ_OK;
    if (top_k == 0) {
        if (out_counts) std::memset(out_counts, 0, nq * 4);
        return RBQ_OK;
    }
    if (top_k > kBfTopKMax) return fail(RBQ_INVALID_CONFIG, "top_k > 16384 is not supported by the brute-force index");
    if (nq >= (1ull << 31)) return fail(RBQ_INVALID_CONFIG, "nq >= 2^31");
    if (!queries || !out_ids || !out_scores || !out_counts) return fail(RBQ_INVALID_CONFIG, "null buffer");
    DeviceGuard g(ix->device);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    return bf_search_impl(ix, queries, nq, top_k, filter_words, filter_nbits, out_ids, out_scores, out_counts);
    RBQ_GUARD_END
}
} // extern "C"
