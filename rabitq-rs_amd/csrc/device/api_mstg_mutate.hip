// api_mstg_mutate.hip — rbq_mstg_append / rbq_mstg_remove_ids (include/rbq_mstg_mutate.h): a new posting-list
// handle that holds an existing one's slots and those of `count` more rows, or all but those whose id is in a set.  The append is
// rbq_index_append's shape (api_append.hip) with the closure in place of the nearest list: pass 1 runs closure_device against the
// handle's own centroids and counts the (row, list) pairs per list; the host plans the grown geometry; append_grow carries the old
// arrays (rnorm with them); pass 2 walks the pairs in chunks of whole rows through encode_rows_at_cursors, every list's cursor
// starting at its old size; the finish is the streamed builder's.  The removal is remove_ids_core (api_remove.hip) behind its own
// argument checks.
#include "api.hpp"
#include "rbq_mstg.h"

using namespace rbq_api;

namespace rbq_api {
namespace {
std::atomic<uint64_t> g_mstg_append_passes{0}; // rbq_debug_mstg_append_passes

// what both calls refuse before they look at their own arguments; no HIP call
int check_handle(const rbq_index* idx, rbq_index** out, const char* ivf_call, const char* what) {
    if (!out) return fail(RBQ_INVALID_CONFIG, "null out pointer");
    *out = nullptr;
    if (!idx || idx->reps.empty()) return fail(RBQ_INVALID_CONFIG, "null index");
    const Replica* old = idx->reps[0];
    if (old->rotator != RBQ_ROTATOR_NONE) return fail(RBQ_INVALID_CONFIG, std::string("not a posting-list handle: use ") + ivf_call);
    if (!old->has_rnorm || !old->has_recon)
        return fail(RBQ_INVALID_CONFIG, std::string("the handle holds no residual norms or reconstruction factors (rbq_index_create*): the ") +
                                            what + " index could not be saved");
    return RBQ_OK;
}

int append_impl(const rbq_index* idx, const float* vectors, uint64_t count, uint64_t first_id, float epsilon, uint32_t max_replicas,
                uint64_t max_chunk_rows, uint32_t* out_lists, uint32_t* out_counts, rbq_index** out) {
    int rc = check_handle(idx, out, "rbq_index_append", "grown");
    if (rc) return rc;
    Replica* old = idx->reps[0];
    if (!vectors) return fail(RBQ_INVALID_CONFIG, "null vectors");
    if (count == 0) return fail(RBQ_INVALID_CONFIG, "no vectors");
    if (max_replicas == 0) return fail(RBQ_INVALID_CONFIG, "max_replicas must be positive");
    if (max_replicas > kMstgMaxReplicas) return fail(RBQ_INVALID_CONFIG, "max_replicas above 64 is not supported");
    if (!(epsilon >= 0.0f) || !std::isfinite(epsilon)) return fail(RBQ_INVALID_CONFIG, "closure epsilon must be finite and not negative");
    if (!out_lists != !out_counts) return fail(RBQ_INVALID_CONFIG, "out_lists and out_counts must be given together");
    const bool out_dev = out_lists && is_device_pointer(out_lists);
    if (out_lists && out_dev != is_device_pointer(out_counts))
        return fail(RBQ_INVALID_CONFIG, "out_lists and out_counts must both be host or both be device memory");
    if (count > 0xfffffff0ull) return fail(RBQ_INVALID_CONFIG, "too many vectors for 32-bit slots");
    // the handle remembers what its lists were encoded with
    const bool opt = !old->tc_some && old->ex_bits > 0;
    const float t_const = old->tc_some ? old->tc_value : 0.0f;
    const int dev = old->device;
    const std::vector<int> devs{dev};

    DeviceGuard g(dev);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    uint64_t bound = 0;
    if ((rc = id_bound_of(old, &bound))) return rc;
    if (first_id < bound)
        return fail(RBQ_INVALID_CONFIG, "first_id " + std::to_string(first_id) + " is below the index's id bound " + std::to_string(bound));
    if (first_id + count < first_id) return fail(RBQ_INVALID_CONFIG, "the new ids pass 2^64 - 1");

    const uint32_t D = old->D, Dc = old->Dc, dim = old->dim, nlist = (uint32_t)old->n_lists, M = max_replicas;
    const bool vec_dev = is_device_pointer(vectors);
    Scratch t; // the closure's output, the pair tables and the block tables: freed on every exit
    EncodeScratch sc;

    // ---- pass 1: the closure of every row against the handle's centroids (chunked and checked for non-finite values inside),
    // the pairs of the whole call, the count per list
    uint32_t *d_lists = nullptr, *d_counts = nullptr;
    HIP_TRY(t.alloc(&d_lists, count * M * 4));
    HIP_TRY(t.alloc(&d_counts, count * 4));
    {
        ClosureArgs a{};
        a.centroids = (const float*)old->centroids.p; a.k = nlist; a.dim = dim; a.data = vectors; a.n = count; a.epsilon = epsilon;
        a.max_replicas = M; a.max_chunk_rows = max_chunk_rows; a.out_lists = d_lists; a.out_counts = d_counts;
        if ((rc = run_closure(a, dev, true))) return rc;
    }
    std::vector<uint32_t> off(count + 1); // first pair of every row
    uint64_t pairs = 0;
    {
        HIP_TRY(hipMemcpy(off.data(), d_counts, count * 4, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < count; ++i) {
            const uint32_t c = off[i];
            if (c > M) return fail(RBQ_IO, "internal error: a closure row longer than max_replicas");
            off[i] = (uint32_t)pairs; pairs += c;
            if (pairs > 0xfffffff0ull) return fail(RBQ_INVALID_CONFIG, "too many (vector, list) pairs for 32-bit slots");
        }
        off[count] = (uint32_t)pairs;
    }
    std::vector<uint64_t> added(nlist);
    {
        Scratch t1; // the pairs of the whole call: only counted
        uint32_t *d_off = nullptr, *d_pl = nullptr, *d_pv = nullptr, *d_cnt = nullptr;
        HIP_TRY(t1.alloc(&d_off, count * 4));
        HIP_TRY(t1.alloc(&d_pl, pairs * 4));
        HIP_TRY(t1.alloc(&d_pv, pairs * 4));
        HIP_TRY(t1.alloc(&d_cnt, (size_t)(nlist + 1) * 4));
        HIP_TRY(hipMemcpy(d_off, off.data(), count * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(d_cnt, 0, (size_t)(nlist + 1) * 4));
        HIP_TRY(launch_closure_expand(d_lists, d_counts, d_off, count, M, d_pl, d_pv, 0));
        HIP_TRY(launch_count_assign(d_pl, pairs, nlist, d_cnt, d_cnt + nlist, 0));
        std::vector<uint32_t> hc((size_t)nlist + 1);
        HIP_TRY(hipMemcpy(hc.data(), d_cnt, hc.size() * 4, hipMemcpyDeviceToHost));
        if (hc[nlist]) return fail(RBQ_IO, "internal error: a closure list out of range");
        std::copy(hc.begin(), hc.begin() + nlist, added.begin());
    }

    // ---- the grown geometry, the old arrays carried into it
    rbq_host::AppendPlan plan;
    {
        std::string detail;
        if (!rbq_host::append_plan(old->h_list_n.data(), added.data(), nlist, &plan, &detail)) return fail(RBQ_INVALID_CONFIG, detail);
        if (plan.old_blocks != old->n_blocks) return fail(RBQ_IO, "internal error: the handle's block count does not match its list sizes");
        if (plan.new_blocks * 32u > 0xfffffff0ull) return fail(RBQ_INVALID_CONFIG, "index too large for 32-bit vector slots");
    }
    ReplicaOwner own{nullptr};
    uint32_t *d_block_list = nullptr, *d_block_nv = nullptr, *d_cursor = nullptr, *d_chunk_first = nullptr;
    if ((rc = append_grow(old, plan, t, own, &d_block_list, &d_block_nv))) return rc;
    Replica* ix = own.ix;

    // ---- pass 2: the pairs in chunks of whole rows, sized by PAIRS (the scratch holds one rotated row per pair) and by
    // max_chunk_rows; a chunk's pairs are expanded again with chunk-local rows, ascending, so every list stays in id order
    const uint64_t PSUB = encode_chunk_rows(D); // (>= 1024 > max_replicas: a row always fits)
    uint64_t RSUB = PSUB;
    if (max_chunk_rows) RSUB = std::min<uint64_t>(RSUB, max_chunk_rows);
    uint32_t *d_coff = nullptr, *d_cpl = nullptr, *d_cpv = nullptr;
    HIP_TRY(t.alloc(&d_coff, std::min<uint64_t>(RSUB, count) * 4));
    HIP_TRY(t.alloc(&d_cpl, std::min<uint64_t>(PSUB, pairs) * 4));
    HIP_TRY(t.alloc(&d_cpv, std::min<uint64_t>(PSUB, pairs) * 4));
    HIP_TRY(t.alloc(&d_cursor, (size_t)nlist * 4));
    HIP_TRY(t.alloc(&d_chunk_first, (size_t)nlist * 4));
    HIP_TRY(hipMemcpy(d_cursor, plan.cursor.data(), (size_t)nlist * 4, hipMemcpyHostToDevice));
    std::vector<uint32_t> coff;
    for (uint64_t r0 = 0; r0 < count;) {
        uint64_t r1 = r0;
        while (r1 < count && r1 - r0 < RSUB && (uint64_t)off[r1 + 1] - off[r0] <= PSUB) ++r1;
        const uint32_t nr = (uint32_t)(r1 - r0), np = off[r1] - off[r0];
        if (nr == 0) return fail(RBQ_IO, "internal error: a row with more pairs than an encode chunk holds");
        if (np) {
            const float* d_vec = vectors + r0 * dim;
            if (!vec_dev) {
                if ((rc = sc.vec.ensure((size_t)nr * dim * 4))) return rc;
                HIP_TRY(hipMemcpy(sc.vec.p, vectors + r0 * dim, (size_t)nr * dim * 4, hipMemcpyHostToDevice));
                d_vec = (const float*)sc.vec.p;
            }
            coff.resize(nr);
            for (uint32_t i = 0; i < nr; ++i) coff[i] = off[r0 + i] - off[r0];
            HIP_TRY(hipMemcpy(d_coff, coff.data(), (size_t)nr * 4, hipMemcpyHostToDevice));
            HIP_TRY(launch_closure_expand(d_lists + r0 * M, d_counts + r0, d_coff, nr, M, d_cpl, d_cpv, 0));
            g_mstg_append_passes.fetch_add(1, std::memory_order_relaxed);
            if ((rc = encode_rows_at_cursors(ix, sc, d_vec, d_cpl, np, first_id + r0, opt, t_const, d_block_list, d_cursor, d_chunk_first,
                                             d_cpv)))
                return rc;
        }
        r0 = r1;
    }

    // ---- finish, as the streamed builder's
    HIP_TRY(launch_block_summary((const uint8_t*)ix->blocks.p, d_block_nv, (uint32_t)plan.new_blocks, Dc, (BlockSummary*)ix->bsum.p, 0));
    HIP_TRY(hipDeviceSynchronize());
    if ((rc = finish_replica(ix, plan.new_n))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (out_lists) {
        const hipMemcpyKind kind = out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        HIP_TRY(hipMemcpy(out_lists, d_lists, count * M * 4, kind));
        HIP_TRY(hipMemcpy(out_counts, d_counts, count * 4, kind));
    }
    ix->opt.numeric_variant = old->opt.numeric_variant;
    ix->id_bound = first_id + count;
    ix->idb_ready = true;
    return wrap_and_replicate(own.release(), devs, out);
}

int remove_impl(const rbq_index* idx, const uint64_t* ids, uint64_t n_ids, uint64_t* out_removed, rbq_index** out) {
    int rc = check_handle(idx, out, "rbq_index_remove_ids", "shrunk");
    if (rc) return rc;
    if (!ids) return fail(RBQ_INVALID_CONFIG, "null ids");
    if (n_ids == 0) return fail(RBQ_INVALID_CONFIG, "no ids");
    const std::vector<int> devs{idx->reps[0]->device};
    return remove_ids_core(idx, ids, n_ids, devs, out_removed, out);
}
} // namespace
} // namespace rbq_api

extern "C" {
int rbq_mstg_append(const rbq_index* idx, const float* vectors, uint64_t count, uint64_t first_id, float closure_epsilon,
                    uint32_t max_replicas, uint64_t max_chunk_rows, uint32_t* out_lists, uint32_t* out_counts, rbq_index** out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return append_impl(idx, vectors, count, first_id, closure_epsilon, max_replicas, max_chunk_rows, out_lists, out_counts, out);
    RBQ_GUARD_END
}

int rbq_mstg_remove_ids(const rbq_index* idx, const uint64_t* ids, uint64_t n_ids, uint64_t* out_removed, rbq_index** out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return remove_impl(idx, ids, n_ids, out_removed, out);
    RBQ_GUARD_END
}

uint64_t rbq_debug_mstg_append_passes(void) { return g_mstg_append_passes.load(std::memory_order_relaxed); }
} // extern "C"
