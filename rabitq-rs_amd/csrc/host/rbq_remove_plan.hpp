// rbq_remove_plan.hpp — the geometry of rbq_index_remove_ids, pure C++: from the list sizes of an index and
// the number of vectors every list keeps, the sizes and first blocks of the shrunk index, and the checks.  Survivors keep their
// order inside a list and lists stay in order, so block j of a list is its j-th run of 32 survivors: the rank of a kept slot
// among its list's kept slots (remove_rank) decides the slot it moves to (remove_dst_slot).
// Shared by api_remove.hip (host), k_remove.hip (the two functions, on the device) and tests/removecheck_main.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "rbq_index_layout.hpp"

#if defined(__HIPCC__)
#define RBQ_REMOVE_HD __host__ __device__
#else
#define RBQ_REMOVE_HD
#endif

namespace rbq_host {

constexpr uint32_t kRemoveNoSlot = 0xffffffffu; // a slot of the shrunk index that no old slot moves into: a pad

// Rank of the kept slot `lane` of an old block among the kept slots of its list.  kept_before / kept_before_list: kept slots in
// all blocks before this one / before the list's first block (the exclusive scan of the per-block kept counts); mask: the block's
// keep mask, bit v = lane v stays.
RBQ_REMOVE_HD inline uint32_t remove_rank(uint32_t kept_before, uint32_t kept_before_list, uint32_t mask, uint32_t lane) {
    return kept_before - kept_before_list + (uint32_t)__builtin_popcount(mask & ((1u << lane) - 1u));
}

// The slot of the shrunk index that the survivor of rank `rank` of a list moves to, gb0_new being the list's first block there.
RBQ_REMOVE_HD inline uint32_t remove_dst_slot(uint32_t gb0_new, uint32_t rank) { return gb0_new * 32u + rank; }

struct RemovePlan {
    std::vector<uint32_t> new_n;   // [n_lists] vectors per list afterwards (= the kept counts)
    std::vector<uint32_t> new_gb0; // [n_lists] first block of every list afterwards: prefix sum of ceil(n / 32)
    std::vector<uint32_t> old_gb0; // [n_lists] first block of every list before
    uint64_t old_blocks = 0, new_blocks = 0, old_vectors = 0, new_vectors = 0;
};

// false (with *detail) when a list is said to keep more vectors than it holds or the old index passes 2^32 vector slots
inline bool remove_plan(const uint32_t* old_n, const uint32_t* kept, size_t n_lists, RemovePlan* out, std::string* detail) {
    size_t ok = 0; // lists before the first one that would keep too many vectors
    while (ok < n_lists && kept[ok] <= old_n[ok]) ++ok;
    // (the slots of the lists before it are checked first: the first failure in list order is the one reported)
    ListLayout before, after;
    if (!list_layout(old_n, ok, &before, detail) || !list_layout(kept, ok, &after, detail)) return false;
    if (ok < n_lists) {
        if (detail) *detail = "list " + std::to_string(ok) + " would keep more vectors than it holds";
        return false;
    }
    RemovePlan p;
    p.new_n.assign(kept, kept + n_lists);
    p.old_gb0 = std::move(before.gb0); p.new_gb0 = std::move(after.gb0);
    p.old_blocks = before.blocks; p.new_blocks = after.blocks; p.old_vectors = before.vectors; p.new_vectors = after.vectors;
    *out = std::move(p);
    return true;
}

} // namespace rbq_host
