// api_append.hip — rbq_index_append / rbq_index_id_bound (include/rbq_append.h): a new handle that holds an
// existing index's vectors and `count` more.  Pass 1 finds the list of every new row (given, or the nearest rotated centroid) and
// counts; the host plans the grown geometry (csrc/host/rbq_append_plan.hpp); one kernel carries the old arrays into it; pass 2 is
// the streamed builder's encoder with every list's cursor starting at its old size; the finish is the streamed builder's.
#include "api.hpp"
#include "../host/rbq_append_plan.hpp"

using namespace rbq_api;

namespace rbq_api {
namespace {
std::atomic<uint64_t> g_append_passes{0}; // rbq_debug_append_passes
std::atomic<uint64_t> g_carry_ns{0};      // rbq_debug_append_carry_ns: device time of the last carry kernel

struct AssignOwner { // frees the assignment workspace on every exit
    AppendAssign* a = nullptr;
    ~AssignOwner() { append_assign_free(a); }
    void reset() { append_assign_free(a); a = nullptr; }
};

} // namespace

// 1 + the largest stored id of the handle (first replica), computed once
int id_bound_of(Replica* ix, uint64_t* out) {
    std::lock_guard<std::mutex> lk(ix->idb_mu);
    if (!ix->idb_ready) {
        DeviceGuard g(ix->device);
        if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
        unsigned long long h = 0;
        if (ix->n_blocks) {
            Scratch t;
            uint32_t* d_nv = nullptr;
            unsigned long long* d_out = nullptr;
            HIP_TRY(t.alloc(&d_nv, ix->n_blocks * 4));
            HIP_TRY(t.alloc(&d_out, 8));
            HIP_TRY(hipMemset(d_out, 0, 8));
            HIP_TRY(launch_load_block_nv((const uint32_t*)ix->list_gb0.p, (const uint32_t*)ix->list_n.p, (uint32_t)ix->n_lists, d_nv, 0));
            HIP_TRY(launch_append_id_bound((const uint64_t*)ix->ids.p, d_nv, ix->n_blocks, d_out, 0));
            HIP_TRY(hipMemcpy(&h, d_out, 8, hipMemcpyDeviceToHost));
        }
        ix->id_bound = h;
        ix->idb_ready = true;
    }
    *out = ix->id_bound;
    return RBQ_OK;
}

// The replica of the grown geometry: arrays allocated, the old ones carried over (api.hpp)
int append_grow(Replica* old, const rbq_host::AppendPlan& plan, Scratch& t, ReplicaOwner& own, uint32_t** d_block_list,
                uint32_t** d_block_nv) {
    rbq_header hdr{};
    hdr.dim = old->dim; hdr.padded_dim = old->D; hdr.metric = old->metric; hdr.rotator = old->rotator; hdr.ex_bits = old->ex_bits;
    hdr.n_lists = old->n_lists;
    const int dev = old->device;
    int rc;
    own.ix = new_replica(&hdr, dev);
    Replica* ix = own.ix;
    const uint64_t nblocks = plan.new_blocks;
    for (Arr Replica::*m : {&Replica::rot_blob, &Replica::centroids}) { // bit for bit those of the old handle
        if ((rc = alloc_arr(ix->*m, (old->*m).bytes))) return rc;
        if ((old->*m).bytes) HIP_TRY(hipMemcpy((ix->*m).p, (old->*m).p, (old->*m).bytes, hipMemcpyDeviceToDevice));
    }
    // (rnorm: an MSTG handle keeps what the `.mstg` format stores beyond the search's arrays)
    if ((rc = alloc_index_arrays(ix, plan.new_n, plan.new_gb0, nblocks, plan.new_vectors, /*recon=*/true, old->has_rnorm))) return rc;
    if (old->has_rnorm) { ix->tc_some = old->tc_some; ix->tc_value = old->tc_value; }
    const rbq_host::IndexBytes B = index_bytes_of(ix);
    const size_t dev_stride = B.block_stride, exd = B.ex_slot;

    if ((rc = upload_block_tables(plan.new_n, plan.new_gb0, nblocks, t, d_block_list, d_block_nv))) return rc;
    AppendCarryParams P{};
    P.block_list = *d_block_list;
    P.gb0_new = (const uint32_t*)ix->list_gb0.p; P.gb0_old = (const uint32_t*)old->list_gb0.p; P.n_old = (const uint32_t*)old->list_n.p;
    P.nb_new = (uint32_t)nblocks; P.nb_old = (uint32_t)old->n_blocks;
    P.rec16 = (uint32_t)(dev_stride / 16); P.ex16 = (uint32_t)(exd * 32 / 16);
    P.src = slot_arrays(old); P.dst = slot_arrays(ix);
    EventPair ev;
    ev.start();
    HIP_TRY(launch_append_carry(P, dev, 0));
    ev.stop();
    uint64_t ns = 0;
    if (ev.ns(&ns)) g_carry_ns.store(ns, std::memory_order_relaxed);
    return RBQ_OK;
}

namespace {
int append_impl(const rbq_index* idx, const float* vectors, const uint32_t* assign, uint64_t count, uint64_t first_id, int rescale,
                float t_const, uint64_t max_chunk_rows, int n_devices, const int* devices, uint32_t* out_assign, rbq_index** out) {
    if (!out) return fail(RBQ_INVALID_CONFIG, "null out pointer");
    *out = nullptr;
    if (!idx || idx->reps.empty()) return fail(RBQ_INVALID_CONFIG, "null index");
    Replica* old = idx->reps[0];
    if (old->rotator == RBQ_ROTATOR_NONE) return fail(RBQ_INVALID_CONFIG, "posting-list handles (RBQ_ROTATOR_NONE) cannot be appended to");
    if (!old->has_recon)
        return fail(RBQ_INVALID_CONFIG, "the handle has no reconstruction factors (rbq_index_create): the grown index could not be saved");
    if (!vectors) return fail(RBQ_INVALID_CONFIG, "null vectors");
    if (count == 0) return fail(RBQ_INVALID_CONFIG, "no vectors");
    if (count > 0xffffffffull || old->n_vectors + count > 0xffffffffull) // (every vector takes a slot; the plan checks the padded total)
        return fail(RBQ_INVALID_CONFIG, "index too large for 32-bit vector slots");
    rbq_header hdr{};
    hdr.dim = old->dim; hdr.padded_dim = old->D; hdr.metric = old->metric; hdr.rotator = old->rotator; hdr.ex_bits = old->ex_bits;
    hdr.n_lists = old->n_lists;
    const int opt = rescale_mode(rescale, &hdr);
    if (opt < 0) return RBQ_INVALID_CONFIG;
    if (!opt && hdr.ex_bits > 0 && !(t_const > 0.0f)) return fail(RBQ_INVALID_CONFIG, "the device encoder needs the constant rescale factor (faster config)");
    const int dev = old->device;
    std::vector<int> devs;
    int rc;
    if (n_devices <= 1 && !devices) devs.push_back(dev);
    else if ((rc = resolve_devices(n_devices, devices, devs))) return rc;
    if (devs[0] != dev) return fail(RBQ_INVALID_CONFIG, "devices[0] must be the device of the index's first replica");

    DeviceGuard g(dev);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    uint64_t bound = 0;
    if ((rc = id_bound_of(old, &bound))) return rc;
    if (first_id < bound)
        return fail(RBQ_INVALID_CONFIG, "first_id " + std::to_string(first_id) + " is below the index's id bound " + std::to_string(bound));
    if (first_id + count < first_id) return fail(RBQ_INVALID_CONFIG, "the new ids pass 2^64 - 1");

    const uint32_t D = old->D, Dc = old->Dc, dim = old->dim, nlist = (uint32_t)old->n_lists;
    const bool vec_dev = is_device_pointer(vectors);
    uint64_t SUB = encode_chunk_rows(D);
    if (max_chunk_rows) SUB = std::min<uint64_t>(SUB, (std::min<uint64_t>(max_chunk_rows, ~0ull - 63) + 63) & ~63ull);
    Scratch t;
    EncodeScratch sc;

    // ---- pass 1: the list of every row on the device, and the count per list
    const uint32_t* d_assign = nullptr;
    if (assign) {
        if (is_device_pointer(assign)) d_assign = assign;
        else {
            uint32_t* p = nullptr;
            HIP_TRY(t.alloc(&p, count * 4));
            HIP_TRY(hipMemcpy(p, assign, count * 4, hipMemcpyHostToDevice));
            d_assign = p;
        }
    } else {
        // half the encode chunk: rotated rows (256 MiB), the staged host rows (256 MiB) and the assignment workspace (512 MiB)
        const uint64_t S1 = std::max<uint64_t>(64, (SUB / 2 + 63) & ~63ull);
        uint32_t *p = nullptr, *d_flag = nullptr;
        HIP_TRY(t.alloc(&p, count * 4));
        HIP_TRY(t.alloc(&d_flag, 4));
        AssignOwner as;
        HIP_TRY(append_assign_create(std::min<uint64_t>(S1, (count + 63) & ~63ull), nlist, D, dev, &as.a));
        for (uint64_t s0 = 0; s0 < count; s0 += S1) {
            const uint32_t n = (uint32_t)std::min<uint64_t>(S1, count - s0);
            const float* d_vec = vectors + s0 * dim;
            if (!vec_dev) {
                if ((rc = sc.vec.ensure((size_t)n * dim * 4))) return rc;
                HIP_TRY(hipMemcpy(sc.vec.p, vectors + s0 * dim, (size_t)n * dim * 4, hipMemcpyHostToDevice));
                d_vec = (const float*)sc.vec.p;
            }
            bool bad = false;
            HIP_TRY(nonfinite_sync(d_vec, (uint64_t)n * dim, d_flag, 0, &bad));
            if (bad) return fail(RBQ_INVALID_CONFIG, "vectors hold a non-finite value (the nearest-centroid assignment needs finite input)");
            if ((rc = sc.rows.ensure((size_t)n * D * 4))) return rc;
            HIP_TRY(launch_rotate_rows(d_vec, nullptr, n, dim, D, (int)old->rotator, (const uint8_t*)old->rot_blob.p, old->trunc, old->fac,
                                       (float*)sc.rows.p, 0));
            HIP_TRY(append_assign_run(as.a, (const float*)sc.rows.p, n, (const float*)old->centroids.p, p + s0, 0));
            HIP_TRY(hipDeviceSynchronize()); // the staging buffers are reused by the next chunk
        }
        d_assign = p;
    }
    std::vector<uint64_t> added(nlist);
    {
        uint32_t* d_counts = nullptr;
        HIP_TRY(t.alloc(&d_counts, (size_t)(nlist + 1) * 4));
        HIP_TRY(hipMemset(d_counts, 0, (size_t)(nlist + 1) * 4));
        HIP_TRY(launch_count_assign(d_assign, count, nlist, d_counts, d_counts + nlist, 0));
        std::vector<uint32_t> hc((size_t)nlist + 1);
        HIP_TRY(hipMemcpy(hc.data(), d_counts, hc.size() * 4, hipMemcpyDeviceToHost));
        if (hc[nlist]) return fail(RBQ_INVALID_CONFIG, "assignment out of range");
        std::copy(hc.begin(), hc.begin() + nlist, added.begin());
    }

    // ---- the grown geometry
    rbq_host::AppendPlan plan;
    {
        std::string detail;
        if (!rbq_host::append_plan(old->h_list_n.data(), added.data(), nlist, &plan, &detail)) return fail(RBQ_INVALID_CONFIG, detail);
        if (plan.old_blocks != old->n_blocks) return fail(RBQ_IO, "internal error: the handle's block count does not match its list sizes");
    }
    ReplicaOwner own{nullptr};
    uint32_t *d_block_list = nullptr, *d_block_nv = nullptr, *d_cursor = nullptr, *d_chunk_first = nullptr;
    if ((rc = append_grow(old, plan, t, own, &d_block_list, &d_block_nv))) return rc;
    Replica* ix = own.ix;
    const uint64_t nblocks = plan.new_blocks;

    // ---- pass 2: the streamed builder's encoder, every list's cursor at its old size
    HIP_TRY(t.alloc(&d_cursor, (size_t)nlist * 4));
    HIP_TRY(t.alloc(&d_chunk_first, (size_t)nlist * 4));
    HIP_TRY(hipMemcpy(d_cursor, plan.cursor.data(), (size_t)nlist * 4, hipMemcpyHostToDevice));
    for (uint64_t s0 = 0; s0 < count; s0 += SUB) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(SUB, count - s0);
        const float* d_vec = vectors + s0 * dim;
        if (!vec_dev) {
            if ((rc = sc.vec.ensure((size_t)n * dim * 4))) return rc;
            HIP_TRY(hipMemcpy(sc.vec.p, vectors + s0 * dim, (size_t)n * dim * 4, hipMemcpyHostToDevice));
            d_vec = (const float*)sc.vec.p;
        }
        g_append_passes.fetch_add(1, std::memory_order_relaxed);
        if ((rc = encode_rows_at_cursors(ix, sc, d_vec, d_assign + s0, n, first_id + s0, opt != 0, t_const, d_block_list, d_cursor,
                                         d_chunk_first)))
            return rc;
    }

    // ---- finish, as the streamed builder's
    HIP_TRY(launch_block_summary((const uint8_t*)ix->blocks.p, d_block_nv, (uint32_t)nblocks, Dc, (BlockSummary*)ix->bsum.p, 0));
    HIP_TRY(hipDeviceSynchronize());
    if ((rc = finish_replica(ix, plan.new_n))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (out_assign) HIP_TRY(hipMemcpy(out_assign, d_assign, count * 4, is_device_pointer(out_assign) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    ix->opt.numeric_variant = old->opt.numeric_variant;
    ix->id_bound = first_id + count;
    ix->idb_ready = true;
    return wrap_and_replicate(own.release(), devs, out);
}
} // namespace
} // namespace rbq_api

extern "C" {
int rbq_index_append(const rbq_index* idx, const float* vectors, const uint32_t* assign, uint64_t count, uint64_t first_id, int rescale,
                     float t_const, uint64_t max_chunk_rows, int n_devices, const int* devices, uint32_t* out_assign, rbq_index** out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return append_impl(idx, vectors, assign, count, first_id, rescale, t_const, max_chunk_rows, n_devices, devices, out_assign, out);
    RBQ_GUARD_END
}

int rbq_index_id_bound(const rbq_index* idx, uint64_t* out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    if (!idx || idx->reps.empty() || !out) return fail(RBQ_INVALID_CONFIG, "null index or out pointer");
    return id_bound_of(idx->reps[0], out);
    RBQ_GUARD_END
}

uint64_t rbq_debug_append_passes(void) { return g_append_passes.load(std::memory_order_relaxed); }
uint64_t rbq_debug_append_carry_ns(void) { return g_carry_ns.load(std::memory_order_relaxed); }
} // extern "C"
