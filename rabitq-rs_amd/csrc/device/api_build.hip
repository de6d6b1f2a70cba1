// api_build.hip — device encoders: the one-shot build from device-resident vectors and the streamed builder
// (rbq_build_stream_*), plus the rescale, k-means and CRC entry points.
#include "api.hpp"

using namespace rbq_api;

// ---- streamed build: the same encoder fed chunk by chunk (rbq_build_stream_*) -----------------------------------
struct rbq_builder {
    Replica* ix = nullptr;
    int device = 0;
    float t_const = 0.0f;
    bool opt = false; // per-vector rescale factor (RBQ_RESCALE_OPTIMAL with ex_bits > 0)
    std::vector<uint32_t> ln, gb0;
    uint64_t n_total = 0, pushed = 0, next_id = 0;
    uint32_t *d_cursor = nullptr, *d_chunk_first = nullptr, *d_block_list = nullptr, *d_block_nv = nullptr, *d_counts = nullptr;
    EncodeScratch sc;
    Scratch tables;
    ~rbq_builder() { if (ix) free_replica(ix); } // (deleted under a DeviceGuard of `device`: the scratch is freed there)
};

namespace rbq_api {
namespace {
// ---- GPU-side encoder: the device analogue of train_with_clusters' quantisation loop ------------------------------
// rotated centroids + list geometry + final arrays of an index that the encoder fills (shared by the one-shot and the
// streamed build).  `ln` = vectors per list; rnorm: the handle keeps every slot's residual norm (a posting-list handle).
int encoder_prepare(Replica* ix, const rbq_header* hdr, const float* centroids, const std::vector<uint32_t>& ln,
                    std::vector<uint32_t>& gb0, bool zero_fill, bool rnorm) {
    const uint32_t D = ix->D, dim = ix->dim, nlist = (uint32_t)ix->n_lists;
    int rc;
    if ((rc = upload_arr(ix->rot_blob, hdr->rotator_blob, hdr->rotator_len))) return rc;
    {
        Scratch t;
        float* d_craw = nullptr;
        HIP_TRY(t.alloc(&d_craw, (size_t)nlist * dim * 4));
        HIP_TRY(hipMemcpy(d_craw, centroids, (size_t)nlist * dim * 4, hipMemcpyHostToDevice));
        if ((rc = alloc_arr(ix->centroids, (size_t)nlist * D * 4))) return rc;
        HIP_TRY(launch_rotate_rows(d_craw, nullptr, nlist, dim, D, (int)ix->rotator, (const uint8_t*)ix->rot_blob.p, ix->trunc, ix->fac,
                                   (float*)ix->centroids.p, 0));
        HIP_TRY(hipDeviceSynchronize());
    }
    rbq_host::ListLayout lay;
    {
        std::string detail;
        if (!rbq_host::list_layout(ln.data(), ln.size(), &lay, &detail)) return fail(RBQ_INVALID_CONFIG, detail);
    }
    gb0 = std::move(lay.gb0);
    if ((rc = alloc_index_arrays(ix, ln, gb0, lay.blocks, lay.vectors, /*recon=*/true, rnorm))) return rc;
    const rbq_host::IndexBytes B = index_bytes_of(ix);
    HIP_TRY(hipMemset(ix->blocks.p, 0, B.blocks));
    if (zero_fill) { // streamed build: padding slots are never visited by the scatter kernels
        HIP_TRY(hipMemset(ix->ids.p, 0xff, B.ids));
        if (B.ex) HIP_TRY(hipMemset(ix->ex.p, 0, B.ex));
        if (ix->ex_bits) { HIP_TRY(hipMemset(ix->fadd_ex.p, 0, B.fadd_ex)); HIP_TRY(hipMemset(ix->fres_ex.p, 0, B.fres_ex)); }
        HIP_TRY(hipMemset(ix->delta.p, 0, B.delta)); HIP_TRY(hipMemset(ix->vl.p, 0, B.vl));
    }
    return RBQ_OK;
}

} // namespace

// block -> list and block -> number of real vectors, on the device
int upload_block_tables(const std::vector<uint32_t>& ln, const std::vector<uint32_t>& gb0, uint64_t nblocks, Scratch& t,
                        uint32_t** d_block_list, uint32_t** d_block_nv) {
    std::vector<uint32_t> bl, bn;
    rbq_host::block_tables(ln, gb0, nblocks, &bl, &bn);
    HIP_TRY(t.alloc(d_block_list, nblocks * 4)); HIP_TRY(t.alloc(d_block_nv, nblocks * 4));
    HIP_TRY(hipMemcpy(*d_block_list, bl.data(), nblocks * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(*d_block_nv, bn.data(), nblocks * 4, hipMemcpyHostToDevice));
    return RBQ_OK;
}

int encode_rows_at_cursors(Replica* ix, EncodeScratch& sc, const float* d_vec, const uint32_t* d_asg, uint32_t n, uint64_t id_base,
                           bool opt, float t_const, const uint32_t* d_block_list, uint32_t* d_cursor, uint32_t* d_chunk_first,
                           const uint32_t* d_pair_row) {
    const uint32_t D = ix->D, Dc = ix->Dc, dim = ix->dim, nlist = (uint32_t)ix->n_lists;
    unsigned bits = 1;
    while ((1ull << bits) < nlist) ++bits;
    int rc;
    if ((rc = sc.ko.ensure((size_t)n * 4)) || (!d_pair_row && (rc = sc.vi.ensure((size_t)n * 4))) || (rc = sc.vo.ensure((size_t)n * 4)) ||
        (rc = sc.row_src.ensure((size_t)n * 4)) || (rc = sc.row_slot.ensure((size_t)n * 4)) ||
        (rc = sc.rows.ensure((size_t)n * D * 4)) || (rc = sc.raw.ensure(ix->ex_bits ? (size_t)n * D : 16)) ||
        (opt && (rc = sc.trow.ensure((size_t)n * 8))))
        return rc;
    if (!d_pair_row) HIP_TRY(launch_iota((uint32_t*)sc.vi.p, n, 0));
    const uint32_t* d_src = d_pair_row ? d_pair_row : (const uint32_t*)sc.vi.p; // the source row of every entry, ascending
    size_t tb = 0;
    HIP_TRY(sort_pairs_u32(nullptr, &tb, d_asg, (uint32_t*)sc.ko.p, d_src, (uint32_t*)sc.vo.p, n, bits, 0));
    if ((rc = sc.tmp.ensure(tb))) return rc;
    HIP_TRY(sort_pairs_u32(sc.tmp.p, &tb, d_asg, (uint32_t*)sc.ko.p, d_src, (uint32_t*)sc.vo.p, n, bits, 0));
    HIP_TRY(launch_chunk_first((const uint32_t*)sc.ko.p, n, d_chunk_first, 0));
    HIP_TRY(launch_chunk_slots((const uint32_t*)sc.ko.p, (const uint32_t*)sc.vo.p, n, (const uint32_t*)ix->list_gb0.p, d_cursor,
                               d_chunk_first, (uint32_t*)sc.row_src.p, (uint32_t*)sc.row_slot.p, 0));
    HIP_TRY(launch_rotate_rows(d_vec, (const uint32_t*)sc.row_src.p, n, dim, D, (int)ix->rotator, (const uint8_t*)ix->rot_blob.p,
                               ix->trunc, ix->fac, (float*)sc.rows.p, 0));
    if (opt)
        HIP_TRY(launch_rescale((const float*)sc.rows.p, (const float*)ix->centroids.p, d_block_list, (const uint32_t*)sc.row_slot.p,
                               (const uint32_t*)sc.row_src.p, n, D, (uint32_t)ix->ex_bits, false, (double*)sc.trow.p, 0));
    EncodeParams P;
    P.rows = (const float*)sc.rows.p; P.centroids = (const float*)ix->centroids.p; P.slot_src = (const uint32_t*)sc.row_src.p;
    P.block_list = d_block_list; P.row_slot = (const uint32_t*)sc.row_slot.p; P.t_row = opt ? (const double*)sc.trow.p : nullptr;
    P.blocks = (uint8_t*)ix->blocks.p; P.raw_ex = (uint8_t*)sc.raw.p;
    P.f_add_ex = (float*)ix->fadd_ex.p; P.f_rescale_ex = (float*)ix->fres_ex.p; P.ids = (uint64_t*)ix->ids.p;
    P.delta = (float*)ix->delta.p; P.vl = (float*)ix->vl.p;
    if (ix->has_rnorm) P.residual_norm = (float*)ix->rnorm.p; // (an MSTG handle: slot order, like delta)
    P.src_base = id_base; P.nslots = n; P.D = D; P.Dc = Dc; P.ex_bits = ix->ex_bits; P.metric = ix->metric; P.t_const = t_const;
    HIP_TRY(launch_encode(P, 0));
    if (ix->ex_bits)
        HIP_TRY(launch_pack_ex((const uint8_t*)sc.raw.p, (const uint32_t*)sc.row_src.p, (const uint32_t*)sc.row_slot.p, n, D,
                               (uint32_t)ix->ex_bits, (uint8_t*)ix->ex.p, 0));
    HIP_TRY(launch_chunk_advance((const uint32_t*)sc.ko.p, n, d_chunk_first, d_cursor, 0));
    HIP_TRY(hipDeviceSynchronize()); // the scratch (and a host caller's buffers) are reused by the next sub-chunk
    return RBQ_OK;
}

// The encoder over n (vector, list) pairs: pair j stores vector d_vec[j] (null: vector j, one list per vector) in list
// d_assign[j].  The pairs arrive in ascending vector order, so the stable sort leaves every list in ascending vector index.
int build_device_pairs(const rbq_header* hdr, const float* centroids, const float* d_data, const uint32_t* d_assign,
                       const uint32_t* d_vec, uint64_t n, int rescale, float t_const, int dev, rbq_index** out) {
    if (!out) return fail(RBQ_INVALID_CONFIG, "null out pointer");
    *out = nullptr;
    int rc = validate_header(hdr);
    if (rc) return rc;
    if (!centroids || !d_data || !d_assign) return fail(RBQ_INVALID_CONFIG, "null buffer");
    if (n == 0) return fail(RBQ_INVALID_CONFIG, "no vectors");
    if (n > 0xfffffff0ull) return fail(RBQ_INVALID_CONFIG, "too many vectors for 32-bit slots");
    const int opt = rescale_mode(rescale, hdr);
    if (opt < 0) return RBQ_INVALID_CONFIG;
    if (!opt && hdr->ex_bits > 0 && !(t_const > 0.0f)) return fail(RBQ_INVALID_CONFIG, "the device encoder needs the constant rescale factor (faster config)");
    std::vector<int> devs;
    if ((rc = resolve_devices(1, &dev, devs))) return rc;
    DeviceGuard g(dev);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");

    ReplicaOwner own{new_replica(hdr, dev)};
    Replica* ix = own.ix;
    const uint32_t D = ix->D, Dc = ix->Dc, dim = ix->dim, nlist = (uint32_t)ix->n_lists;
    Scratch t;

    // list sizes
    std::vector<uint32_t> ln(nlist), gb0;
    {
        uint32_t* d_counts = nullptr;
        HIP_TRY(t.alloc(&d_counts, (size_t)(nlist + 1) * 4));
        HIP_TRY(hipMemset(d_counts, 0, (size_t)(nlist + 1) * 4));
        HIP_TRY(launch_count_assign(d_assign, n, nlist, d_counts, d_counts + nlist, 0));
        std::vector<uint32_t> hc((size_t)nlist + 1);
        HIP_TRY(hipMemcpy(hc.data(), d_counts, hc.size() * 4, hipMemcpyDeviceToHost));
        if (hc[nlist]) return fail(RBQ_INVALID_CONFIG, "assignment out of range");
        std::copy(hc.begin(), hc.begin() + nlist, ln.begin());
    }
    // (a posting-list handle keeps what the `.mstg` format stores beyond the search's arrays)
    if ((rc = encoder_prepare(ix, hdr, centroids, ln, gb0, /*zero_fill=*/false, /*rnorm=*/ix->rotator == RBQ_ROTATOR_NONE))) return rc;
    const rbq_host::IndexBytes B = index_bytes_of(ix);
    const uint64_t nblocks = ix->n_blocks, nslots = B.slots;
    const size_t dev_stride = B.block_stride, exd = B.ex_slot;
    if (ix->has_rnorm) {
        ix->tc_some = !opt && ix->ex_bits > 0; // RabitqConfig::faster: Some(t_const) unless 1-bit; RabitqConfig::new: None
        ix->tc_value = ix->tc_some ? t_const : 0.0f;
    }
    std::vector<uint64_t> vstart(nlist);
    { uint64_t run = 0; for (uint32_t c = 0; c < nlist; ++c) { vstart[c] = run; run += ln[c]; } }

    // stable grouping by list (ascending vector index inside a list, src/ivf.rs:1141-1149): radix sort on the list id
    uint32_t* d_slot_src = nullptr;
    {
        uint32_t *d_ko = nullptr, *d_vi = nullptr, *d_vo = nullptr;
        uint64_t* d_vstart = nullptr;
        HIP_TRY(t.alloc(&d_ko, n * 4)); HIP_TRY(t.alloc(&d_vo, n * 4));
        if (!d_vec) HIP_TRY(t.alloc(&d_vi, n * 4));
        HIP_TRY(t.alloc(&d_vstart, (size_t)nlist * 8));
        HIP_TRY(hipMemcpy(d_vstart, vstart.data(), (size_t)nlist * 8, hipMemcpyHostToDevice));
        if (!d_vec) HIP_TRY(launch_iota(d_vi, n, 0));
        const uint32_t* d_src = d_vec ? d_vec : d_vi;
        unsigned bits = 1;
        while ((1ull << bits) < nlist) ++bits;
        size_t tb = 0;
        HIP_TRY(sort_pairs_u32(nullptr, &tb, d_assign, d_ko, d_src, d_vo, (size_t)n, bits, 0));
        void* d_tmp = nullptr;
        HIP_TRY(t.alloc(&d_tmp, tb));
        HIP_TRY(sort_pairs_u32(d_tmp, &tb, d_assign, d_ko, d_src, d_vo, (size_t)n, bits, 0));
        HIP_TRY(t.alloc(&d_slot_src, nslots * 4));
        HIP_TRY(hipMemset(d_slot_src, 0xff, nslots * 4));
        HIP_TRY(launch_scatter_slots(d_ko, d_vo, n, (const uint32_t*)ix->list_gb0.p, d_vstart, d_slot_src, 0));
    }
    uint32_t *d_block_list = nullptr, *d_block_nv = nullptr;
    if ((rc = upload_block_tables(ln, gb0, nblocks, t, &d_block_list, &d_block_nv))) return rc;

    // encode, a chunk of blocks at a time (scratch: rotated rows + raw ex codes of the chunk)
    {
        uint64_t chunk_blocks = std::max<uint64_t>(2, ((512ull << 20) / ((size_t)D * 4) / 32) & ~1ull);
        chunk_blocks = std::min<uint64_t>(chunk_blocks, (nblocks + 1) & ~1ull);
        const uint64_t chunk_slots = chunk_blocks * 32;
        float* d_rows = nullptr;
        uint8_t* d_raw = nullptr;
        double* d_t = nullptr;
        HIP_TRY(t.alloc(&d_rows, chunk_slots * D * 4));
        HIP_TRY(t.alloc(&d_raw, ix->ex_bits ? chunk_slots * D : 16));
        if (opt) HIP_TRY(t.alloc(&d_t, chunk_slots * 8));
        for (uint64_t b0 = 0; b0 < nblocks; b0 += chunk_blocks) {
            const uint64_t nb = std::min<uint64_t>(chunk_blocks, nblocks - b0), ns = nb * 32, s0 = b0 * 32;
            HIP_TRY(launch_rotate_rows(d_data, d_slot_src + s0, (uint32_t)ns, dim, D, (int)ix->rotator, (const uint8_t*)ix->rot_blob.p,
                                       ix->trunc, ix->fac, d_rows, 0));
            if (opt)
                HIP_TRY(launch_rescale(d_rows, (const float*)ix->centroids.p, d_block_list + b0, nullptr, d_slot_src + s0, (uint32_t)ns, D,
                                       (uint32_t)ix->ex_bits, false, d_t, 0));
            EncodeParams P;
            P.rows = d_rows; P.centroids = (const float*)ix->centroids.p; P.slot_src = d_slot_src + s0; P.block_list = d_block_list + b0;
            P.row_slot = nullptr; P.t_row = d_t;
            P.blocks = (uint8_t*)ix->blocks.p + b0 * dev_stride; P.raw_ex = d_raw;
            P.f_add_ex = (float*)ix->fadd_ex.p + s0; P.f_rescale_ex = (float*)ix->fres_ex.p + s0; P.ids = (uint64_t*)ix->ids.p + s0;
            P.delta = (float*)ix->delta.p + s0; P.vl = (float*)ix->vl.p + s0;
            if (ix->has_rnorm) P.residual_norm = (float*)ix->rnorm.p + s0;
            P.src_base = 0; P.nslots = (uint32_t)ns; P.D = D; P.Dc = Dc; P.ex_bits = ix->ex_bits; P.metric = ix->metric; P.t_const = t_const;
            HIP_TRY(launch_encode(P, 0));
            if (ix->ex_bits)
                HIP_TRY(launch_pack_ex(d_raw, d_slot_src + s0, nullptr, (uint32_t)ns, D, (uint32_t)ix->ex_bits, (uint8_t*)ix->ex.p + s0 * exd, 0));
        }
        HIP_TRY(launch_block_summary((const uint8_t*)ix->blocks.p, d_block_nv, (uint32_t)nblocks, Dc, (BlockSummary*)ix->bsum.p, 0));
        HIP_TRY(hipDeviceSynchronize());
    }
    if ((rc = finish_replica(ix, ln))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return wrap_and_replicate(own.release(), devs, out);
}

namespace {
int build_device_impl(const rbq_header* hdr, const float* centroids, const float* d_data, const uint32_t* d_assign,
                      uint64_t n, int rescale, float t_const, int dev, rbq_index** out) {
    return build_device_pairs(hdr, centroids, d_data, d_assign, nullptr, n, rescale, t_const, dev, out);
}
void free_builder(rbq_builder* b) {
    if (!b) return;
    DeviceGuard g(b->device);
    delete b;
}


int stream_begin_impl(const rbq_header* hdr, const float* centroids, const uint32_t* list_sizes, int rescale, float t_const,
                      int dev, rbq_builder** out) {
    if (!out) return fail(RBQ_INVALID_CONFIG, "null out pointer");
    *out = nullptr;
    int rc = validate_header(hdr);
    if (rc) return rc;
    if (!centroids || !list_sizes) return fail(RBQ_INVALID_CONFIG, "null buffer");
    const int opt = rescale_mode(rescale, hdr);
    if (opt < 0) return RBQ_INVALID_CONFIG;
    if (!opt && hdr->ex_bits > 0 && !(t_const > 0.0f)) return fail(RBQ_INVALID_CONFIG, "the device encoder needs the constant rescale factor (faster config)");
    std::vector<int> devs;
    if ((rc = resolve_devices(1, &dev, devs))) return rc;
    DeviceGuard g(dev);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    std::unique_ptr<rbq_builder> b(new rbq_builder());
    b->device = dev; b->t_const = t_const; b->opt = opt != 0;
    b->ix = new_replica(hdr, dev);
    const uint32_t nlist = (uint32_t)hdr->n_lists;
    b->ln.assign(list_sizes, list_sizes + nlist);
    for (uint32_t c = 0; c < nlist; ++c) b->n_total += b->ln[c];
    if (b->n_total == 0) return fail(RBQ_INVALID_CONFIG, "no vectors");
    if ((rc = encoder_prepare(b->ix, hdr, centroids, b->ln, b->gb0, /*zero_fill=*/true, /*rnorm=*/false))) return rc;
    if ((rc = upload_block_tables(b->ln, b->gb0, b->ix->n_blocks, b->tables, &b->d_block_list, &b->d_block_nv))) return rc;
    HIP_TRY(b->tables.alloc(&b->d_cursor, (size_t)nlist * 4));
    HIP_TRY(b->tables.alloc(&b->d_chunk_first, (size_t)nlist * 4));
    HIP_TRY(b->tables.alloc(&b->d_counts, (size_t)(nlist + 1) * 4));
    HIP_TRY(hipMemset(b->d_cursor, 0, (size_t)nlist * 4));
    HIP_TRY(hipMemset(b->d_counts, 0, (size_t)(nlist + 1) * 4));
    *out = b.release();
    return RBQ_OK;
}

int stream_push_impl(rbq_builder* b, const float* vectors, const uint32_t* assign, uint64_t first_id, uint64_t count) {
    if (!b || !b->ix) return fail(RBQ_INVALID_CONFIG, "null builder");
    if (count == 0) return RBQ_OK;
    if (!vectors || !assign) return fail(RBQ_INVALID_CONFIG, "null buffer");
    if (first_id < b->next_id) return fail(RBQ_INVALID_CONFIG, "chunks must be pushed in ascending id order (list membership order, src/ivf.rs:1141-1149)");
    if (b->pushed + count > b->n_total) return fail(RBQ_INVALID_CONFIG, "more vectors pushed than the list sizes announced");
    DeviceGuard g(b->device);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    Replica* ix = b->ix;
    const uint32_t dim = ix->dim, nlist = (uint32_t)ix->n_lists;
    const bool vec_dev = is_device_pointer(vectors), asg_dev = is_device_pointer(assign);
    // sub-chunks bounded by the scratch for the rotated rows (512 MB)
    const uint64_t SUB = encode_chunk_rows(ix->D);
    int rc;
    for (uint64_t s0 = 0; s0 < count; s0 += SUB) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(SUB, count - s0);
        const float* d_vec = vectors + s0 * dim;
        const uint32_t* d_asg = assign + s0;
        if (!vec_dev) {
            if ((rc = b->sc.vec.ensure((size_t)n * dim * 4))) return rc;
            HIP_TRY(hipMemcpy(b->sc.vec.p, vectors + s0 * dim, (size_t)n * dim * 4, hipMemcpyHostToDevice));
            d_vec = (const float*)b->sc.vec.p;
        }
        if (!asg_dev) {
            if ((rc = b->sc.assign.ensure((size_t)n * 4))) return rc;
            HIP_TRY(hipMemcpy(b->sc.assign.p, assign + s0, (size_t)n * 4, hipMemcpyHostToDevice));
            d_asg = (const uint32_t*)b->sc.assign.p;
        }
        // counts so far incl. this sub-chunk: no list may outgrow its announced size (its slots are fixed)
        HIP_TRY(launch_count_assign(d_asg, n, nlist, b->d_counts, b->d_counts + nlist, 0));
        {
            std::vector<uint32_t> hc((size_t)nlist + 1);
            HIP_TRY(hipMemcpy(hc.data(), b->d_counts, hc.size() * 4, hipMemcpyDeviceToHost));
            if (hc[nlist]) return fail(RBQ_INVALID_CONFIG, "assignment out of range");
            for (uint32_t c = 0; c < nlist; ++c)
                if (hc[c] > b->ln[c]) return fail(RBQ_INVALID_CONFIG, "list " + std::to_string(c) + " received more vectors than announced");
        }
        if ((rc = encode_rows_at_cursors(ix, b->sc, d_vec, d_asg, n, first_id + s0, b->opt, b->t_const, b->d_block_list, b->d_cursor,
                                         b->d_chunk_first)))
            return rc;
    }
    b->pushed += count;
    b->next_id = first_id + count;
    return RBQ_OK;
}

int stream_finish_impl(rbq_builder* b, int n_devices, const int* devices, rbq_index** out) {
    if (!out) return fail(RBQ_INVALID_CONFIG, "null out pointer");
    *out = nullptr;
    if (!b || !b->ix) return fail(RBQ_INVALID_CONFIG, "null builder");
    if (b->pushed != b->n_total) return fail(RBQ_INVALID_CONFIG, "list sizes do not match the pushed vectors");
    std::vector<int> devs;
    int rc;
    if (n_devices <= 1 && !devices) devs.push_back(b->device);
    else if ((rc = resolve_devices(n_devices, devices, devs))) return rc;
    if (devs[0] != b->device) return fail(RBQ_INVALID_CONFIG, "devices[0] must be the device the builder was opened on");
    DeviceGuard g(b->device);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    Replica* ix = b->ix;
    HIP_TRY(launch_block_summary((const uint8_t*)ix->blocks.p, b->d_block_nv, (uint32_t)ix->n_blocks, ix->Dc, (BlockSummary*)ix->bsum.p, 0));
    HIP_TRY(hipDeviceSynchronize());
    if ((rc = finish_replica(ix, b->ln))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    b->ix = nullptr;
    return wrap_and_replicate(ix, devs, out);
}
} // namespace
} // namespace rbq_api

extern "C" {
int rbq_index_build_device(const rbq_header* hdr, const float* centroids, const float* d_data, const uint32_t* d_assign,
                           uint64_t n, float t_const, int device, rbq_index** out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return build_device_impl(hdr, centroids, d_data, d_assign, n, RBQ_RESCALE_CONST, t_const, device, out);
    RBQ_GUARD_END
}
int rbq_index_build_device_ex(const rbq_header* hdr, const float* centroids, const float* d_data, const uint32_t* d_assign,
                              uint64_t n, int rescale, float t_const, int device, rbq_index** out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return build_device_impl(hdr, centroids, d_data, d_assign, n, rescale, t_const, device, out);
    RBQ_GUARD_END
}

int rbq_build_stream_begin(const rbq_header* hdr, const float* centroids, const uint32_t* list_sizes, float t_const, int device,
                           rbq_builder** out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return stream_begin_impl(hdr, centroids, list_sizes, RBQ_RESCALE_CONST, t_const, device, out);
    RBQ_GUARD_END
}
int rbq_build_stream_begin_ex(const rbq_header* hdr, const float* centroids, const uint32_t* list_sizes, int rescale,
                              float t_const, int device, rbq_builder** out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return stream_begin_impl(hdr, centroids, list_sizes, rescale, t_const, device, out);
    RBQ_GUARD_END
}
int rbq_debug_best_rescale(const float* o_abs, uint64_t n, uint32_t dim, uint32_t ex_bits, int device, double* out_t) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    if (!o_abs || !out_t) return fail(RBQ_INVALID_CONFIG, "null buffer");
    if (dim == 0 || dim > 2048) return fail(RBQ_INVALID_CONFIG, "dim must be in 1..2048");
    if (ex_bits == 0 || ex_bits > 7) return fail(RBQ_INVALID_CONFIG, "ex_bits must be in 1..7");
    for (uint64_t i = 0; i < n * dim; ++i) // o = |r| / norm(r): the window bound of k_rescale relies on o <= 1
        if (!(o_abs[i] >= 0.0f && o_abs[i] <= 1.0f)) return fail(RBQ_INVALID_CONFIG, "o_abs must lie in [0, 1]");
    if (n == 0) return RBQ_OK;
    std::vector<int> devs;
    int rc;
    if ((rc = resolve_devices(1, &device, devs))) return rc;
    DeviceGuard g(device);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    const uint64_t chunk = std::max<uint64_t>(1, (256ull << 20) / ((uint64_t)dim * 4));
    Scratch t;
    float* d_o = nullptr;
    double* d_t = nullptr;
    const uint64_t rows = std::min(chunk, n);
    HIP_TRY(t.alloc(&d_o, rows * dim * 4));
    HIP_TRY(t.alloc(&d_t, rows * 8));
    for (uint64_t r0 = 0; r0 < n; r0 += chunk) {
        const uint64_t nr = std::min(chunk, n - r0);
        HIP_TRY(hipMemcpy(d_o, o_abs + r0 * dim, nr * dim * 4, hipMemcpyHostToDevice));
        HIP_TRY(launch_rescale(d_o, nullptr, nullptr, nullptr, nullptr, (uint32_t)nr, dim, ex_bits, true, d_t, 0));
        HIP_TRY(hipMemcpy(out_t + r0, d_t, nr * 8, hipMemcpyDeviceToHost));
    }
    return RBQ_OK;
    RBQ_GUARD_END
}
int rbq_kmeans_device(const float* d_data, uint64_t n, uint32_t dim, uint64_t k, uint64_t niter, uint64_t nredo, uint64_t seed,
                      int spherical, uint64_t max_points_per_centroid, uint64_t decode_block_size, int device, float* centroids,
                      uint32_t* d_assignments, double* objective, uint64_t* stats) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    // validate_inputs (src/kmeans.rs) with the crate's messages, then what this project adds
    if (n == 0) return fail(RBQ_INVALID_CONFIG, "k-means requires non-empty data");
    if (k == 0) return fail(RBQ_INVALID_CONFIG, "k must be positive");
    if (niter == 0) return fail(RBQ_INVALID_CONFIG, "max_iter must be positive");
    if (k > n) return fail(RBQ_INVALID_CONFIG, "k cannot exceed number of samples");
    if (nredo == 0) return fail(RBQ_INVALID_CONFIG, "nredo must be positive");
    if (decode_block_size == 0) return fail(RBQ_INVALID_CONFIG, "decode_block_size must be positive");
    if (dim == 0) return fail(RBQ_INVALID_CONFIG, "vectors must have at least one dimension");
    if (n >= 0xffffffffull) return fail(RBQ_INVALID_CONFIG, "k-means supports fewer than 2^32 - 1 vectors");
    if (!d_data || !centroids || !d_assignments || !objective) return fail(RBQ_INVALID_CONFIG, "null buffer");
    std::vector<int> devs;
    int rc;
    if ((rc = resolve_devices(1, &device, devs))) return rc;
    DeviceGuard g(device);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    KMeansArgs a{d_data, n, dim, k, niter, nredo, seed, spherical, max_points_per_centroid, decode_block_size, device, centroids,
                 d_assignments, objective, stats};
    std::string detail;
    rc = kmeans_device(a, detail);
    return rc ? fail(rc, detail) : RBQ_OK;
    RBQ_GUARD_END
}
uint64_t rbq_debug_set_kmeans_chunk_rows(uint64_t rows) { return g_km_chunk_rows_cap.exchange(rows, std::memory_order_relaxed); }
uint64_t rbq_debug_kmeans_assign_passes(void) { return g_km_assign_passes.load(std::memory_order_relaxed); }
int rbq_debug_gemm_shortlist_front(const float* centroids, uint64_t k, uint32_t dim, const float* rows, uint64_t n, int device,
                                   float* out_dots, float* out_nx, float* out_nc, float* out_ncmax, uint16_t* out_row_hi,
                                   uint16_t* out_row_lo, uint16_t* out_cent_hi, uint16_t* out_cent_lo) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    if (k == 0 || k > 0xffffffffull) return fail(RBQ_INVALID_CONFIG, "k must be in 1..2^32 - 1");
    if (dim == 0 || dim > 0xffffffe0u) return fail(RBQ_INVALID_CONFIG, "dim must be in 1..2^32 - 32");
    if (!centroids || !out_nc || !out_ncmax || (n && (!rows || !out_dots || !out_nx))) return fail(RBQ_INVALID_CONFIG, "null buffer");
    if (!out_row_hi != !out_row_lo || !out_cent_hi != !out_cent_lo) return fail(RBQ_INVALID_CONFIG, "hi and lo images go together");
    std::vector<int> devs;
    int rc;
    if ((rc = resolve_devices(1, &device, devs))) return rc;
    DeviceGuard g(device);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    FrontTapArgs a{centroids, k, dim, rows, n, out_dots, out_nx, out_nc, out_ncmax, out_row_hi, out_row_lo, out_cent_hi, out_cent_lo};
    std::string detail;
    rc = gemm_shortlist_front_tap(a, device, detail);
    return rc ? fail(rc, detail) : RBQ_OK;
    RBQ_GUARD_END
}
int rbq_build_stream_push(rbq_builder* b, const float* vectors, const uint32_t* assign, uint64_t first_id, uint64_t count) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return stream_push_impl(b, vectors, assign, first_id, count);
    RBQ_GUARD_END
}
int rbq_build_stream_finish(rbq_builder* b, int n_devices, const int* devices, rbq_index** out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    int rc = stream_finish_impl(b, n_devices, devices, out);
    if (rc == RBQ_OK) free_builder(b);
    return rc;
    RBQ_GUARD_END
}
void rbq_build_stream_abort(rbq_builder* b) { try { free_builder(b); } catch (...) {} }


int rbq_debug_crc32_device(const void* d_bytes, uint64_t len, int device, uint32_t* out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    if (!out || (len && !d_bytes)) return fail(RBQ_INVALID_CONFIG, "null buffer");
    std::vector<int> devs;
    int rc = resolve_devices(1, &device, devs);
    if (rc) return rc;
    DeviceGuard g(device);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    if (len) { // the range must lie inside one device allocation
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)d_bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(RBQ_INVALID_CONFIG, "not a device allocation");
        }
        if ((const uint8_t*)d_bytes + len > (const uint8_t*)base + size) return fail(RBQ_INVALID_CONFIG, "range exceeds the allocation");
    }
    Scratch t;
    uint32_t *d_seg = nullptr, *d_out = nullptr;
    HIP_TRY(t.alloc(&d_seg, crc_scratch_words(len) * 4));
    HIP_TRY(t.alloc(&d_out, 4));
    HIP_TRY(launch_crc32((const uint8_t*)d_bytes, len, d_seg, d_out, 0));
    HIP_TRY(hipMemcpy(out, d_out, 4, hipMemcpyDeviceToHost));
    return RBQ_OK;
    RBQ_GUARD_END
}
} // extern "C"
