// rbq_bf_plan.hpp — the plan of ONE brute-force call (api_bf.hip: rbq_bf_search_batch, rbq_bf_range_batch, rbq_bf_range_exact_batch):
// how many vectors a chunk of the distance workspace holds, how many chunks the index makes, how many queries a sub-batch takes
// within the workspace budgets, and what the call's own buffers are sized by.  Every budget is evaluated once, here; the HIP side
// sizes buffers and launches what the plan says.  Pure C++ (no HIP): tests/bfplancheck_main.cpp builds it with
// -fsanitize=address,undefined and tests/test_bf_plan_host.py checks it on the CPU.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace rbq_host {

constexpr uint64_t kBfDistBudget = 128ull << 20; // distance workspace of one sub-batch (bytes)
constexpr uint64_t kBfHeapBudget = 48ull << 20;  // heap workspace (between vector chunks, or for top_k above the LDS heap)
constexpr uint64_t kBfOutBudget = 48ull << 20;   // result buffers of one sub-batch
constexpr uint64_t kBfMaxSubBatch = 1024;
// the kernels' own constants (launch.hpp: kBfLdsHeapMaxTopK, kBfRangeSpan), restated for the host; api_bf.hip asserts they agree
constexpr uint32_t kBfPlanLdsHeapMaxTopK = 8191;
constexpr uint32_t kBfPlanRangeSpan = 2048;

// What the plan reads of a call.  The entries have refused n == 0, nq == 0 and, for a top-k call, top_k == 0.
struct BfCallShape {
    uint64_t n = 0, nq = 0;     // vectors of the index, queries of the call
    bool range = false;         // range search (estimate or exact) instead of top-k
    uint32_t top_k = 0;         // (range: the capacity of a caller's output row, 0 = count only)
    uint64_t chunk_vectors = 0; // rbq_bf_debug_set_chunk_vectors: at most this many vectors per chunk (0: the default)
};

struct BfCallPlan {
    uint64_t nv_chunk = 1; // vectors per chunk of the distance workspace (the last chunk may be shorter)
    uint64_t n_chunks = 1;
    uint64_t sub = 1;      // queries per sub-batch
    // top-k
    bool lds_heap = false; // k_bf_select keeps its heap in the LDS
    bool heap_ws = false;  // ... and needs the heap workspace: between chunks, or for a heap the LDS cannot hold
    // range
    uint64_t cap = 0;      // slots per row on the device: no row holds more than n matches
    uint64_t spans = 0;    // spans of a full chunk (span_counts is sized by it)
};

inline BfCallPlan plan_bf_call(const BfCallShape& s) {
    BfCallPlan p;
    // vector chunks of at most kBfDistBudget / 4 vectors, sub-batches of queries within the workspace budgets
    p.nv_chunk = std::min<uint64_t>({s.n, kBfDistBudget / 4, s.chunk_vectors ? s.chunk_vectors : UINT64_MAX});
    p.n_chunks = (s.n + p.nv_chunk - 1) / p.nv_chunk;
    p.sub = std::min<uint64_t>({s.nq, kBfMaxSubBatch, std::max<uint64_t>(1, kBfDistBudget / (p.nv_chunk * 4))});
    if (s.range) {
        p.spans = (p.nv_chunk + kBfPlanRangeSpan - 1) / kBfPlanRangeSpan;
        p.cap = std::min<uint64_t>(s.top_k, s.n);
        if (p.cap) p.sub = std::min<uint64_t>(p.sub, std::max<uint64_t>(1, kBfOutBudget / (p.cap * 12)));
        return p;
    }
    const uint64_t K = s.top_k;
    p.lds_heap = s.top_k <= kBfPlanLdsHeapMaxTopK;
    p.heap_ws = p.n_chunks > 1 || !p.lds_heap;
    p.sub = std::min<uint64_t>(p.sub, std::max<uint64_t>(1, kBfOutBudget / (K * 12)));
    if (p.heap_ws) p.sub = std::min<uint64_t>(p.sub, std::max<uint64_t>(1, kBfHeapBudget / ((K + 1) * 8)));
    return p;
}

} // namespace rbq_host
