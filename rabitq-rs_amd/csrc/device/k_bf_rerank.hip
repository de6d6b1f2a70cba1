// k_bf_rerank.hip — translation unit of the exact brute-force top-k's kernels (bf_rerank.hpp) and their launchers: six
// instantiations of the score kernel, metric x element type of the raw rows, and the order kernel.  gfx950 only.
#include <hip/hip_runtime.h>

#include "launch_util.hpp" // raw_rows_by_element, dispatch_raw_dtype

#pragma clang fp contract(off)

#include "rerank_score.hpp" // (after the pragma: the scorer's sums are unfused)
#include "bf_rerank.hpp"

namespace rbq {

namespace {
// what both kernels assume of the pool: 1 <= top_k <= pool <= pool_np2 <= kBfRerankPoolMax, pool_np2 a power of two
bool bf_rerank_shape_ok(const BfRerankParams& P) {
    return P.nq != 0u && P.top_k != 0u && P.top_k <= P.pool && P.pool <= P.pool_np2 && P.pool_np2 <= kBfRerankPoolMax &&
           (P.pool_np2 & (P.pool_np2 - 1u)) == 0u && P.pool_ids && P.pool_counts && P.exact;
}
template <int RAW>
hipError_t launch_bfr(const BfRerankParams& P, hipStream_t s) {
    const dim3 grid((P.pool + kBfRerankSlice - 1u) / kBfRerankSlice, P.nq), block(kBfRerankThreads);
    if (P.metric == 1) hipLaunchKernelGGL((k_bf_rerank_score<true, RAW>), grid, block, 0, s, P);
    else hipLaunchKernelGGL((k_bf_rerank_score<false, RAW>), grid, block, 0, s, P);
    return hipGetLastError();
}
} // namespace

hipError_t launch_bf_rerank_score(const BfRerankParams& P0, hipStream_t s) {
    BfRerankParams P = P0;
    if (!bf_rerank_shape_ok(P) || P.dim == 0u || P.dim > kBfRangeExactMaxDim || !P.raw || P.n_raw == 0u || !P.queries) return hipErrorInvalidValue;
    P.raw_by_element = raw_rows_by_element(P.raw, P.raw_dtype, P.dim);
    return dispatch_raw_dtype(P.raw_dtype, [&](auto raw) { return launch_bfr<decltype(raw)::value>(P, s); });
}

// Dynamic LDS of the order kernel: 16 bytes of keys per pool entry (np2) and the count.  At pool 4096: 65552 bytes.
size_t bf_rerank_order_lds_bytes(uint32_t pool_np2) { return (size_t)pool_np2 * 16 + 16; }

hipError_t launch_bf_rerank_order(const BfRerankParams& P, int device, hipStream_t s) {
    static LdsAttrCache attr;
    if (!bf_rerank_shape_ok(P) || !P.out_ids || !P.out_scores || !P.out_counts) return hipErrorInvalidValue;
    const size_t lds = bf_rerank_order_lds_bytes(P.pool_np2);
    if (lds > kLdsPerWorkgroupMax) return hipErrorInvalidValue;
    const hipError_t e = attr.ensure(reinterpret_cast<const void*>(&k_bf_rerank_order), lds, device);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bf_rerank_order, dim3(P.nq), dim3(kBfRerankThreads), lds, s, P);
    return hipGetLastError();
}

} // namespace rbq
