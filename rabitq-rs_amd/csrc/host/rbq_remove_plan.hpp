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
    RemovePlan p;
    p.new_n.resize(n_lists); p.new_gb0.resize(n_lists); p.old_gb0.resize(n_lists);
    for (size_t c = 0; c < n_lists; ++c) {
        if (kept[c] > old_n[c]) {
            if (detail) *detail = "list " + std::to_string(c) + " would keep more vectors than it holds";
            return false;
        }
        p.old_gb0[c] = (uint32_t)p.old_blocks; p.new_gb0[c] = (uint32_t)p.new_blocks;
        p.new_n[c] = kept[c];
        p.old_blocks += ((uint64_t)old_n[c] + 31u) / 32u;
        p.new_blocks += ((uint64_t)kept[c] + 31u) / 32u;
        p.old_vectors += old_n[c];
        p.new_vectors += kept[c];
        if (p.old_blocks * 32u > 0xffffffffull || p.new_blocks * 32u > 0xffffffffull) {
            if (detail) *detail = "index too large for 32-bit vector slots";
            return false;
        }
    }
    *out = std::move(p);
    return true;
}

} // namespace rbq_host
