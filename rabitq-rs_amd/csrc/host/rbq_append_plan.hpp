// rbq_append_plan.hpp — the geometry of rbq_index_append, pure C++: from the list sizes of an index and
// the number of vectors every list receives, the sizes and first blocks of the grown index, where each of its blocks comes from
// and where every list's new vectors start.  A list's block j stays its block j: a list keeps its blocks as one contiguous range
// (a partly filled tail block as it is) and new blocks follow them, so carrying the old index over is whole block ranges.
// Shared by api_append.hip (host), k_append.hip (append_src_block, on the device) and tests/appendcheck_main.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "rbq_index_layout.hpp"

#if defined(__HIPCC__)
#define RBQ_APPEND_HD __host__ __device__
#else
#define RBQ_APPEND_HD
#endif

namespace rbq_host {

constexpr uint32_t kAppendNoBlock = 0xffffffffu; // a block of the grown index that no old block is carried into

// The old block carried into block b of the grown index, b being a block of a list whose first block is gb0_new there and
// gb0_old in the old index, where it holds n_old vectors; kAppendNoBlock for a block the list did not have.
RBQ_APPEND_HD inline uint32_t append_src_block(uint32_t b, uint32_t gb0_new, uint32_t gb0_old, uint32_t n_old) {
    const uint32_t j = b - gb0_new, nb_old = n_old / 32u + (n_old % 32u ? 1u : 0u);
    return j < nb_old ? gb0_old + j : kAppendNoBlock;
}

struct AppendPlan {
    std::vector<uint32_t> new_n;   // [n_lists] vectors per list afterwards
    std::vector<uint32_t> new_gb0; // [n_lists] first block of every list afterwards
    std::vector<uint32_t> old_gb0; // [n_lists] first block of every list before
    std::vector<uint32_t> cursor;  // [n_lists] position inside the list of its first new vector (= its old size)
    uint64_t old_blocks = 0, new_blocks = 0, new_vectors = 0;
};

// false (with *detail) when a list would pass 2^32 - 1 vectors or the index 2^32 vector slots
inline bool append_plan(const uint32_t* old_n, const uint64_t* added, size_t n_lists, AppendPlan* out, std::string* detail) {
    AppendPlan p;
    p.new_n.resize(n_lists); p.cursor.assign(old_n, old_n + n_lists);
    size_t ok = 0; // lists before the first one that would hold too many vectors
    for (; ok < n_lists && added[ok] <= 0xffffffffull && (uint64_t)old_n[ok] + added[ok] <= 0xffffffffull; ++ok)
        p.new_n[ok] = (uint32_t)(old_n[ok] + added[ok]);
    // (the slots of the lists before it are checked first: the first failure in list order is the one reported)
    ListLayout before, after;
    if (!list_layout(old_n, ok, &before, detail) || !list_layout(p.new_n.data(), ok, &after, detail)) return false;
    if (ok < n_lists) {
        if (detail) *detail = "list " + std::to_string(ok) + " would hold more than 2^32 - 1 vectors";
        return false;
    }
    p.old_gb0 = std::move(before.gb0); p.new_gb0 = std::move(after.gb0);
    p.old_blocks = before.blocks; p.new_blocks = after.blocks; p.new_vectors = after.vectors;
    *out = std::move(p);
    return true;
}

} // namespace rbq_host
