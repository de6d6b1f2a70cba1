// rbq_index_layout.hpp — the layout of an IVF replica's device arrays, pure C++: from the list sizes, the
// first block of every list and the totals; from the header's dimensions and the block count, the byte size of every array; the
// block -> list and block -> real vectors tables; the descending prefix sums of the per-list block counts.  Every construction
// path (create, load, build, append, remove, the `.mstg` loader) takes these from here, and so do the readers of the same facts
// (rbq_debug_copy_index, the save and fetch staging).  Shared by the api_*.hip units, rbq_append_plan.hpp, rbq_remove_plan.hpp and
// tests/indexlayout_main.cpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "rbq_scan_limits.hpp"

namespace rbq_host {

constexpr size_t kBlockSummaryBytes = 32; // sizeof(BlockSummary) == sizeof(BlockSummaryEx) (tied to the structs in device/api.hpp)
constexpr size_t kExReadAhead = 256;      // bytes past the last slot's ex codes that the refine loads may read (kept zero)

// 32-vector blocks of a list of n vectors
inline uint64_t blocks_of(uint64_t n) { return (n + 31) / 32; }

struct ListLayout {
    std::vector<uint32_t> gb0; // [n_lists] first block of every list: the prefix sum of blocks_of(n)
    uint64_t blocks = 0, vectors = 0;
};

// false (with *detail; *out untouched) when the lists take more than 2^32 - 1 vector slots
inline bool list_layout(const uint32_t* n, size_t n_lists, ListLayout* out, std::string* detail) {
    ListLayout L;
    L.gb0.resize(n_lists);
    for (size_t c = 0; c < n_lists; ++c) {
        L.gb0[c] = (uint32_t)L.blocks;
        L.blocks += blocks_of(n[c]);
        L.vectors += n[c];
        if (L.blocks * 32 > 0xffffffffull) {
            if (detail) *detail = "index too large for 32-bit vector slots";
            return false;
        }
    }
    *out = std::move(L);
    return true;
}

// Byte sizes of a replica's arrays: the logical size of each (what rbq_debug_copy_index serves), and for `ex` the allocation too.
struct IndexBytes {
    size_t block_stride = 0; // one block record: lane-major sign codes of 32 vectors | f_add[32] | f_rescale[32] | f_error[32]
    size_t ex_slot = 0;      // ex codes of one slot (ex_bytes_dev), 0 at ex_bits 0
    size_t slots = 0;        // n_blocks * 32
    size_t blocks = 0, ids = 0, ex = 0, fadd_ex = 0, fres_ex = 0, bsum = 0, bsumx = 0, lsum = 0, delta = 0, vl = 0, rnorm = 0;
    size_t centroids = 0, cent_hl = 0, cent_f16 = 0, cent_f16_resid = 0, cnorm2 = 0, list_gb0 = 0, list_n = 0;
    size_t ex_alloc = 0;     // `ex` with its read-ahead pad; 0 when there are no ex codes
};

inline IndexBytes index_bytes(uint32_t D, uint32_t Dc, uint32_t ex_bits, uint64_t n_blocks, uint64_t n_lists) {
    IndexBytes b;
    b.block_stride = (size_t)Dc * 4 + 384;
    b.ex_slot = rbq::ex_bytes_dev(D, ex_bits);
    b.slots = (size_t)n_blocks * 32;
    b.blocks = (size_t)n_blocks * b.block_stride;
    b.ids = b.slots * 8;
    b.ex = b.slots * b.ex_slot;
    b.ex_alloc = b.ex_slot ? b.ex + kExReadAhead : 0;
    b.fadd_ex = b.fres_ex = ex_bits ? b.slots * 4 : 0;
    b.bsum = b.bsumx = (size_t)n_blocks * kBlockSummaryBytes;
    b.lsum = (size_t)n_lists * kBlockSummaryBytes;
    b.delta = b.vl = b.rnorm = b.slots * 4;
    b.centroids = b.cent_hl = (size_t)n_lists * D * 4;
    b.cent_f16 = (size_t)n_lists * D * 2;
    b.cent_f16_resid = b.cnorm2 = b.list_gb0 = b.list_n = (size_t)n_lists * 4;
    return b;
}

// block -> list and block -> number of real vectors (1..32) of a layout's n_blocks blocks
inline void block_tables(const std::vector<uint32_t>& ln, const std::vector<uint32_t>& gb0, uint64_t n_blocks,
                         std::vector<uint32_t>* block_list, std::vector<uint32_t>* block_nv) {
    block_list->assign(n_blocks, 0);
    block_nv->assign(n_blocks, 0);
    for (size_t c = 0; c < ln.size(); ++c) {
        const uint32_t nb = (uint32_t)blocks_of(ln[c]);
        for (uint32_t b = 0; b < nb; ++b) {
            (*block_list)[gb0[c] + b] = (uint32_t)c;
            (*block_nv)[gb0[c] + b] = std::min<uint32_t>(32u, ln[c] - b * 32u);
        }
    }
}

// [n_lists + 1] prefix sums of the per-list block counts sorted descending: entry p bounds the blocks of any p lists
inline std::vector<uint64_t> nblk_desc_prefix(const std::vector<uint32_t>& ln) {
    std::vector<uint64_t> nblk(ln.size()), out(ln.size() + 1, 0);
    for (size_t c = 0; c < ln.size(); ++c) nblk[c] = blocks_of(ln[c]);
    std::sort(nblk.begin(), nblk.end(), std::greater<uint64_t>());
    for (size_t c = 0; c < ln.size(); ++c) out[c + 1] = out[c] + nblk[c];
    return out;
}

} // namespace rbq_host
