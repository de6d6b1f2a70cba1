// api_load.hip — rbq_index_load_rbq1_stream (include/rbq_persist.h): rbq_index_load_rbq1 over a reader.  The framing, the span
// cutter and the verdict are the host's (csrc/host/rbq_load_stream.hpp, shared with tests/loadcheck_main.cpp); the spans are
// checksummed (k_save.hip's CRC), checked and scattered into the device layout by the GPU (k_load.hip).  The whole-buffer loader
// (api_index.hip) is left as it is: its handle and its errors are what this one has to equal.
#include "api.hpp"
#include "../host/rbq_load_stream.hpp"

using namespace rbq_api;

namespace rbq_api {
namespace {
std::atomic<uint64_t> g_load_span{0}; // rbq_debug_set_load_span (0: the default)

using rbq_host::LoadFraming;
using rbq_host::LoadPiece;

int load_stream_impl(rbq_read_fn read, void* user, uint64_t total, int n_devices, const int* devices, rbq_index** out) {
    if (!out) return fail(RBQ_INVALID_CONFIG, "null out pointer");
    *out = nullptr;
    if (!read) return fail(RBQ_INVALID_CONFIG, "null reader");
    auto rd = [&](uint64_t off, void* dst, uint64_t n) { return read(user, off, dst, n) == 0; };
    const auto read_failed = [] { return fail(RBQ_IO, "read callback failed"); };

    // ---- 1. framing (host) ------------------------------------------------------------------------------------------------
    LoadFraming F;
    if (!rbq_host::load_frame(rd, total, F)) return read_failed();
    std::string detail;
    bool want_stored = false;
    if (!F.header_ok) { // nothing of the cluster region is known: no prefix can come before this failure
        const int rc = rbq_host::load_verdict_framing(F, rbq_host::kLoadNoBadPrefix, total, &detail, &want_stored);
        return fail(rc, detail);
    }
    const uint64_t budget = rbq_host::load_span_budget(g_load_span.load(std::memory_order_relaxed), F.g);

    // What comes after rbq1_parse in the whole-buffer loader, in its order: validate_header, resolve_devices,
    // create_from_sources' size check.  None of them stops the record pass: a failing check of the stream comes first.
    rbq_header hdr = F.h;
    uint8_t dummy_blob = 0;
    hdr.rotator_blob = &dummy_blob; // (validate_header only asks whether there is one)
    const int vh_rc = validate_header(&hdr);
    const std::string vh_detail = g_err;
    std::vector<int> devs;
    const int dv_rc = resolve_devices(n_devices, devices, devs);
    const std::string dv_detail = g_err;
    int dev = 0;
    if (dv_rc == RBQ_OK) dev = devs[0];
    else HIP_TRY(hipGetDevice(&dev));
    rbq_host::ListLayout lay;
    std::string too_large_detail;
    const bool too_large = !rbq_host::list_layout(F.list_n.data(), F.list_n.size(), &lay, &too_large_detail); // (no early return: below)
    const uint64_t nblocks = lay.blocks;
    // the index is built while the spans pass when the stream is framed to its end and this build can serve it
    const bool scatter = F.complete() && vh_rc == RBQ_OK && dv_rc == RBQ_OK && !too_large;
    const bool want_crc = F.complete();

    DeviceGuard g(dev);
    if (!g.ok) return fail(RBQ_DEVICE, "hipSetDevice failed");

    // header from byte 8 and the rotator: CRC on the host; the blob is kept when the index will need it
    uint32_t crc = 0;
    std::vector<uint8_t> blob;
    if (want_crc) {
        uint8_t head[44];
        if (!rd(0, head, 44)) return read_failed();
        crc = rbq_host::crc32_update(0, head + 8, 36);
        const uint64_t step = std::min<uint64_t>(budget, std::max<uint64_t>(F.h.rotator_len, 1));
        blob.resize(scatter ? F.h.rotator_len : step);
        for (uint64_t o = 0; o < F.h.rotator_len; o += step) {
            const uint64_t n = std::min(step, F.h.rotator_len - o);
            uint8_t* dst = blob.data() + (scatter ? o : 0);
            if (!rd(F.rot_off + o, dst, n)) return read_failed();
            crc = rbq_host::crc32_update(crc, dst, n);
        }
    }

    ReplicaOwner own{nullptr};
    Replica* ix = nullptr;
    Scratch t; // (released before `own`)
    const uint32_t nlist = (uint32_t)F.list_n.size();
    int rc;
    if (scatter) {
        hdr.rotator_blob = blob.data();
        own.ix = ix = new_replica(&hdr, dev);
        if ((rc = upload_arr(ix->rot_blob, blob.data(), F.h.rotator_len))) return rc;
        if ((rc = alloc_index_arrays(ix, F.list_n, lay.gb0, nblocks, F.actual, /*recon=*/true, /*rnorm=*/false))) return rc;
        if ((rc = alloc_arr(ix->centroids, index_bytes_of(ix).centroids))) return rc;
        blob = std::vector<uint8_t>();
    }

    // ---- 2. record pass (GPU): read span k + 1 while the kernels run on span k ----------------------------------------------
    const uint64_t region = F.region_end - F.cluster_begin, cap = std::max<uint64_t>(std::min(budget, region), 16);
    const size_t piece_cap = (size_t)std::min<uint64_t>(rbq_host::kLoadMaxPieces, (uint64_t)F.list_n.size() * rbq_host::kLpSections + 1) * sizeof(LoadPiece);
    uint8_t *pin[2] = {nullptr, nullptr}, *d_span[2] = {nullptr, nullptr};
    LoadPiece *pin_pc[2] = {nullptr, nullptr}, *d_pc[2] = {nullptr, nullptr};
    uint32_t *d_seg = nullptr, *d_crc = nullptr, *h_crc = nullptr;
    unsigned long long *d_bad = nullptr, *h_bad = nullptr;
    hipEvent_t ev[2];
    HIP_TRY(t.make_stream());
    HIP_TRY(t.alloc(&d_seg, crc_scratch_words(cap) * 4));
    HIP_TRY(t.alloc(&d_crc, 2 * 4));
    HIP_TRY(t.alloc(&d_bad, 8));
    HIP_TRY(t.alloc_pinned(&h_crc, 2 * 4));
    HIP_TRY(t.alloc_pinned(&h_bad, 8));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(t.alloc(&d_span[i], cap));
        HIP_TRY(t.alloc_pinned(&pin[i], cap));
        HIP_TRY(t.alloc(&d_pc[i], piece_cap));
        HIP_TRY(t.alloc_pinned(&pin_pc[i], piece_cap));
        HIP_TRY(t.event(&ev[i]));
    }
    HIP_TRY(hipMemsetAsync(d_bad, 0xff, 8, t.stream));

    LoadSpanParams P;
    std::memset(&P, 0, sizeof P);
    P.scatter = scatter ? 1u : 0u; P.D = (uint32_t)F.g.D; P.ex_bits = F.h.ex_bits; P.exb = F.g.exb; P.bad_prefix = d_bad;
    if (scatter) {
        P.Dc = ix->Dc; P.centroids = (uint32_t*)ix->centroids.p; P.blocks = (uint8_t*)ix->blocks.p; P.ids = (uint64_t*)ix->ids.p;
        P.ex = (uint8_t*)ix->ex.p; P.fadd_ex = (uint32_t*)ix->fadd_ex.p; P.fres_ex = (uint32_t*)ix->fres_ex.p;
        P.delta = (uint32_t*)ix->delta.p; P.vl = (uint32_t*)ix->vl.p;
    }
    rbq_host::LoadCutter cut(F, budget);
    std::vector<LoadPiece> pieces;
    uint64_t span_len[2] = {0, 0};
    uint64_t k = 0, folded = 0; // spans issued; spans whose CRC is in `crc`
    auto fold = [&](uint64_t upto) -> int { // CRCs of spans [folded, upto), in order (each waits for its own span)
        for (; folded < upto; ++folded) {
            const int b = (int)(folded & 1);
            HIP_TRY(hipEventSynchronize(ev[b]));
            if (want_crc) crc = rbq_host::crc32_combine(crc, h_crc[b], span_len[b]);
        }
        return RBQ_OK;
    };
    uint64_t s_off = 0, s_len = 0;
    while (cut.next(pieces, &s_off, &s_len)) {
        const int b = (int)(k & 1);
        if (k >= 2 && (rc = fold(k - 1))) return rc; // buffer b is free once span k - 2 is through
        const uint64_t nwg = rbq_host::load_assign_workgroups(pieces, F.h.ex_bits, scatter);
        if (s_len > cap || pieces.size() > rbq_host::kLoadMaxPieces) return fail(RBQ_IO, "internal error: span larger than its buffer");
        if (!rd(s_off, pin[b], s_len)) return read_failed();
        std::memcpy(pin_pc[b], pieces.data(), pieces.size() * sizeof(LoadPiece));
        span_len[b] = s_len;
        HIP_TRY(hipMemcpyAsync(d_span[b], pin[b], s_len, hipMemcpyHostToDevice, t.stream));
        HIP_TRY(hipMemcpyAsync(d_pc[b], pin_pc[b], pieces.size() * sizeof(LoadPiece), hipMemcpyHostToDevice, t.stream));
        if (want_crc) {
            HIP_TRY(launch_crc32(d_span[b], s_len, d_seg, d_crc + b, t.stream));
            HIP_TRY(hipMemcpyAsync(h_crc + b, d_crc + b, 4, hipMemcpyDeviceToHost, t.stream));
        }
        P.span = d_span[b]; P.span_off = s_off; P.pieces = d_pc[b]; P.n_pieces = (uint32_t)pieces.size();
        HIP_TRY(launch_load_span(P, nwg, t.stream));
        HIP_TRY(hipEventRecord(ev[b], t.stream));
        ++k;
    }
    if ((rc = fold(k))) return rc;
    HIP_TRY(hipMemcpyAsync(h_bad, d_bad, 8, hipMemcpyDeviceToHost, t.stream));
    HIP_TRY(hipStreamSynchronize(t.stream));

    // ---- 3. verdict -------------------------------------------------------------------------------------------------------
    rc = rbq_host::load_verdict_framing(F, *h_bad, total, &detail, &want_stored);
    if (rc) return fail(rc, detail);
    uint32_t stored = 0;
    if (!rd(F.body_end, &stored, 4)) return read_failed();
    if ((rc = rbq_host::load_verdict_crc(crc, stored, &detail))) return fail(rc, detail);
    if (vh_rc) return fail(vh_rc, vh_detail);
    if (dv_rc) return fail(dv_rc, dv_detail);
    if (too_large) return fail(RBQ_INVALID_CONFIG, too_large_detail);

    uint32_t* d_bnv = nullptr;
    HIP_TRY(t.alloc(&d_bnv, nblocks * 4));
    HIP_TRY(launch_load_block_nv((const uint32_t*)ix->list_gb0.p, (const uint32_t*)ix->list_n.p, nlist, d_bnv, t.stream));
    HIP_TRY(launch_block_summary((const uint8_t*)ix->blocks.p, d_bnv, (uint32_t)nblocks, ix->Dc, (BlockSummary*)ix->bsum.p, t.stream));
    HIP_TRY(hipStreamSynchronize(t.stream));
    if ((rc = finish_replica(ix, F.list_n))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return wrap_and_replicate(own.release(), devs, out);
}
} // namespace
} // namespace rbq_api

extern "C" {
int rbq_index_load_rbq1_stream(rbq_read_fn read, void* user, uint64_t total_len, int n_devices, const int* devices, rbq_index** out) {
    g_err.clear();
    RBQ_GUARD_BEGIN
    return load_stream_impl(read, user, total_len, n_devices, devices, out);
    RBQ_GUARD_END
}

uint64_t rbq_debug_set_load_span(uint64_t bytes) { return g_load_span.exchange(bytes, std::memory_order_relaxed); }
} // extern "C"
