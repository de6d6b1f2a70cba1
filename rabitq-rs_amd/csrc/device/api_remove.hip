// api_remove.hip — rbq_index_remove_ids (include/rbq_remove.h): a new handle that holds an existing index's
// vectors except those whose id is in a set.  Nothing is encoded again: the set is sorted, one kernel marks the slots that stay,
// a scan ranks them inside their lists, the host plans the shrunk geometry (csrc/host/rbq_remove_plan.hpp), one kernel scatters
// the slot map and one gathers every array through it; the finish is the append's.
#include "api.hpp"
#include "../host/rbq_remove_plan.hpp"

using namespace rbq_api;

namespace rbq_api {
namespace {
std::atomic<uint64_t> g_gather_ns{0}; // rbq_debug_remove_gather_ns: device time of the last gather kernel

int remove_impl(const rbq_index* idx, const uint64_t* ids, uint64_t n_ids, int n_devices, const int* devices, uint64_t* out_removed,
                rbq_index** out) {
    if (!out) return fail(RBQ_INVALID_CONFIG, "null out pointer");
    *out = nullptr;
    if (!idx || idx->reps.empty()) return fail(RBQ_INVALID_CONFIG, "null index");
    Replica* old = idx->reps[0];
    if (old->rotator == RBQ_ROTATOR_NONE) return fail(RBQ_INVALID_CONFIG, "posting-list handles (RBQ_ROTATOR_NONE) cannot be removed from");
    if (!old->has_recon)
        return fail(RBQ_INVALID_CONFIG, "the handle has no reconstruction factors (rbq_index_create): the shrunk index could not be saved");
    if (!ids) return fail(RBQ_INVALID_CONFIG, "null ids");
    if (n_ids == 0) return fail(RBQ_INVALID_CONFIG, "no ids");
    const int dev = old->device;
    std::vector<int> devs;
    int rc;
    if (n_devices <= 1 && !devices) devs.push_back(dev);
    else if ((rc = resolve_devices(n_devices, devices, devs))) return rc;
    if (devs[0] != dev) return fail(RBQ_INVALID_CONFIG, "devices[0] must be the device of the index's first replica");
    return remove_ids_core(idx, ids, n_ids, devs, out_removed, out);
}
} // namespace

// Everything after the argument checks (api.hpp): rbq_index_remove_ids and rbq_mstg_remove_ids
int remove_ids_core(const rbq_index* idx, const uint64_t* ids, uint64_t n_ids, const std::vector<int>& devs, uint64_t* out_removed,
                    rbq_index** out) {
    Replica* old = idx->reps[0];
    const int dev = old->device;
    int rc;
    DeviceGuard g(dev);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");
    rbq_header hdr{};
    hdr.dim = old->dim; hdr.padded_dim = old->D; hdr.metric = old->metric; hdr.rotator = old->rotator; hdr.ex_bits = old->ex_bits;
    hdr.n_lists = old->n_lists;
    const uint32_t Dc = old->Dc, nlist = (uint32_t)old->n_lists;
    const uint64_t nb_old = old->n_blocks;
    Scratch t;

    // ---- mark: the set sorted on the device, one keep mask per old block
    uint32_t *d_bl_old = nullptr, *d_nv_old = nullptr, *d_mask = nullptr, *d_scan = nullptr, *d_kept = nullptr;
    {
        const uint64_t* d_in = ids;
        if (!is_device_pointer(ids)) {
            uint64_t* p = nullptr;
            HIP_TRY(t.alloc(&p, n_ids * 8));
            HIP_TRY(hipMemcpy(p, ids, n_ids * 8, hipMemcpyHostToDevice));
            d_in = p;
        }
        uint64_t* d_set = nullptr;
        void* d_tmp = nullptr;
        size_t tb = 0;
        HIP_TRY(t.alloc(&d_set, n_ids * 8));
        HIP_TRY(sort_keys_u64(nullptr, &tb, d_in, d_set, (size_t)n_ids, 0));
        HIP_TRY(t.alloc(&d_tmp, tb));
        HIP_TRY(sort_keys_u64(d_tmp, &tb, d_in, d_set, (size_t)n_ids, 0));

        rbq_host::ListLayout lay_old;
        if (old->h_list_n.size() != nlist || !rbq_host::list_layout(old->h_list_n.data(), nlist, &lay_old, nullptr) || lay_old.blocks != nb_old)
            return fail(RBQ_IO, "internal error: the handle's block count does not match its list sizes");
        if ((rc = upload_block_tables(old->h_list_n, lay_old.gb0, nb_old, t, &d_bl_old, &d_nv_old))) return rc;
        HIP_TRY(t.alloc(&d_mask, (nb_old + 1) * 4)); // (one entry more: the scan's last value is the total)
        HIP_TRY(t.alloc(&d_scan, (nb_old + 1) * 4));
        HIP_TRY(t.alloc(&d_kept, (size_t)nlist * 4));
        HIP_TRY(hipMemset(d_mask, 0, (nb_old + 1) * 4));
        HIP_TRY(launch_remove_mark((const uint64_t*)old->ids.p, d_nv_old, nb_old, d_set, n_ids, d_mask, 0));
    }

    // ---- rank: kept slots before every block; the kept count of every list goes to the host
    std::vector<uint32_t> kept(nlist);
    {
        void* d_tmp = nullptr;
        size_t tb = 0;
        HIP_TRY(remove_scan_kept(nullptr, &tb, d_mask, d_scan, nb_old + 1, 0));
        HIP_TRY(t.alloc(&d_tmp, tb));
        HIP_TRY(remove_scan_kept(d_tmp, &tb, d_mask, d_scan, nb_old + 1, 0));
        HIP_TRY(launch_remove_list_kept(d_scan, (const uint32_t*)old->list_gb0.p, (const uint32_t*)old->list_n.p, nlist, nb_old, d_kept, 0));
        HIP_TRY(hipMemcpy(kept.data(), d_kept, (size_t)nlist * 4, hipMemcpyDeviceToHost));
    }

    // ---- the shrunk geometry
    rbq_host::RemovePlan plan;
    {
        std::string detail;
        if (!rbq_host::remove_plan(old->h_list_n.data(), kept.data(), nlist, &plan, &detail)) return fail(RBQ_INVALID_CONFIG, detail);
        if (plan.old_blocks != nb_old) return fail(RBQ_IO, "internal error: the handle's block count does not match its list sizes");
    }
    if (plan.new_vectors == 0) // (rbq_index_build_device_ex refuses zero rows too: there is no handle without vectors)
        return fail(RBQ_INVALID_CONFIG, "the ids cover every vector of the index: an index without vectors cannot be built");
    ReplicaOwner own{new_replica(&hdr, dev)};
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
    const size_t dev_stride = B.block_stride, exd = B.ex_slot, nslots = B.slots;

    // ---- the slot map, then the gather
    uint32_t *d_block_list = nullptr, *d_block_nv = nullptr, *d_map = nullptr;
    if ((rc = upload_block_tables(plan.new_n, plan.new_gb0, nblocks, t, &d_block_list, &d_block_nv))) return rc;
    HIP_TRY(t.alloc(&d_map, nslots * 4));
    HIP_TRY(hipMemset(d_map, 0xff, nslots * 4));
    HIP_TRY(launch_remove_slot_map(d_mask, d_scan, d_bl_old, (const uint32_t*)old->list_gb0.p, (const uint32_t*)ix->list_gb0.p, nb_old,
                                   nblocks, d_map, 0));
    {
        RemoveGatherParams P{};
        P.map = d_map; P.nb_new = (uint32_t)nblocks; P.n_slots_old = (uint32_t)(nb_old * 32);
        P.rec = (uint32_t)dev_stride; P.G16 = Dc / 128u; P.tail = Dc % 128u == 64u ? 1u : 0u; P.ex16 = (uint32_t)(exd / 16);
        P.src = slot_arrays(old); P.dst = slot_arrays(ix);
        EventPair ev;
        ev.start();
        HIP_TRY(launch_remove_gather(P, dev, 0));
        ev.stop();
        uint64_t ns = 0;
        if (ev.ns(&ns)) g_gather_ns.store(ns, std::memory_order_relaxed);
    }

    // ---- finish, as the append's
    HIP_TRY(launch_block_summary((const uint8_t*)ix->blocks.p, d_block_nv, (uint32_t)nblocks, Dc, (BlockSummary*)ix->bsum.p, 0));
    HIP_TRY(hipDeviceSynchronize());
    if ((rc = finish_replica(ix, plan.new_n))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    ix->opt.numeric_variant = old->opt.numeric_variant;
    const uint64_t removed = plan.old_vectors - plan.new_vectors;
    if ((rc = wrap_and_replicate(own.release(), devs, out))) return rc;
    if (out_removed) *out_removed = removed;
    return RBQ_OK;
}
} // namespace rbq_api

extern "C" {
int rbq_index_remove_ids(const rbq_index* idx, const uint64_t* ids, uint64_t n_ids, int n_devices, const int* devices,
                         uint64_t* out_removed, rbq_index** out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return remove_impl(idx, ids, n_ids, n_devices, devices, out_removed, out);
    RBQ_GUARD_END
}

uint64_t rbq_debug_remove_gather_ns(void) { return g_gather_ns.load(std::memory_order_relaxed); }
} // extern "C"
