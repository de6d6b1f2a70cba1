/*
 * rbq_mstg_range.h — C ABI of the range search on MSTG handles: every vector of the posting lists that
 * rbq_mstg_search_batch (rbq_mstg.h) selects whose estimate is below a radius, in scan order, optionally one entry per id.
 * No counterpart in lqhl/rabitq-rs.  A header of its own under include/ext/, included as "ext/rbq_mstg_range.h": rbq_mstg.h
 * and the set of headers in include/ itself stay as they are.  The entries are exported by the same library.
 */
#ifndef RBQ_MSTG_RANGE_H
#define RBQ_MSTG_RANGE_H

#include <stdint.h>

#include "../rbq_mstg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The range search: every vector of the selected lists whose estimate is below `radius`, a pure function of
 * what rbq_mstg_search_batch and rbq_posting_scan_batch compute.  Per query:
 *  1. Steps 1 to 3 of rbq_mstg_search_batch select the lists; out_list_ids / out_list_counts are that call's, bit for bit.
 *  2. The candidates are the (list, position) entries of the kept lists in scan order: the lists in selection order, each in its
 *     vector order.  The estimate of a candidate is the value rbq_posting_scan_batch computes for it (step 4 of
 *     rbq_mstg_search_batch): binary estimate, g_add = S or the canonical -dot, a non-finite estimate drops the candidate, an L2
 *     estimate below zero is zero; distances for both metrics.
 *  3. A candidate matches iff estimate < radius, for both metrics.  Every f32 is a legal radius: +inf matches every candidate
 *     that is not dropped; NaN matches nothing, and so does 0 (or less) for L2.
 *  4. distinct == 0: the matches, in scan order.  out_counts[q] is their total and may exceed `capacity` — that is how a short
 *     row shows; the first min(total, capacity) matches are written, the other slots are UINT64_MAX / NaN.  The same call gives
 *     the same rows every time.
 *  5. distinct != 0: among the matches that share an id the one with the smallest estimate by value stays, on equal values the
 *     earlier in scan order (rule 3 of the refined search); the ones that stay keep their scan order.  out_counts[q] is the number
 *     of distinct ids; the first min(that, capacity) are written.  One workgroup orders a query's matches in LDS: a query with
 *     more than RBQ_MSTG_RANGE_DISTINCT_MAX matches (replicas counted) gets out_counts[q] = UINT32_MAX and no entry — nothing is
 *     deduplicated on a prefix.  The caller repeats such a query with distinct == 0 and removes the repeats itself.
 *  6. capacity == 0 or ef_search == 0: RBQ_OK with every count 0, as rbq_mstg_search_batch with top_k == 0; nq == 0: RBQ_OK.
 *   out_ids [nq][capacity] u64, out_scores [nq][capacity] f32, out_counts [nq] u32; the list outputs may be NULL.
 * Errors: those of rbq_mstg_search_batch in its order, with `capacity` where it has top_k (capacity <= 2^20, as the IVF range
 * search); all before the first HIP call.  Host queries are cut into chunks inside the 1 GiB workspace (the rows of step 5 are
 * part of it); the result does not depend on the chunking.  "query_dtype" is honoured as by the other MSTG entries; the IVF
 * options "range_search" / "range_exact" are not read.
 *
 * Exact range search: with rbq_debug_set_option(idx, "mstg_range_exact", 1) (every replica, default 0) and the
 * 32 bits of an f32 x in "mstg_range_exact_bits" (default +inf), both entries read `radius` as the candidate radius r and answer:
 *  a. the candidates of a query are the rows of this call with the option 0 at radius r, distinct != 0 and unlimited capacity —
 *     lists, estimates, the distinct rule and the scan order of steps 1 to 5; the list outputs are that call's, bit for bit.  A
 *     query with more than RBQ_MSTG_RANGE_DISTINCT_MAX matches at r, replicas counted, gets out_counts[q] = UINT32_MAX and no entry;
 *  b. every candidate id is scored as the exact rerank scores it (rbq_mstg.h): canonical l2_distance_sqr, or minus the canonical
 *     dot product, of the caller's unrotated query row and raw row `id` of rbq_index_set_rerank_vectors, 16-bit elements widened;
 *  c. a candidate matches iff that distance is finite and < x, for both metrics: NaN never matches, id >= n_raw never matches, a
 *     NaN x matches nothing;
 *  d. the matches keep the candidates' scan order; out_scores holds the exact distance's bits; out_counts[q] is their total and may
 *     exceed `capacity`, the first min(total, capacity) are written, the other slots are UINT64_MAX / NaN.
 * RBQ_INVALID_CONFIG (detail set), after the errors above and before the first HIP call: distinct == 0 (an exact answer is per
 * id), no raw vectors attached, "rerank" 0 — nothing is silently approximated.  capacity == 0, ef_search == 0 and nq == 0 are as in
 * step 6.  With the option 0 both entries are bit for bit what they are without it. */
#define RBQ_MSTG_RANGE_DISTINCT_MAX 4096
int rbq_mstg_range_batch(const rbq_index* idx, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t capacity,
                         uint32_t ef_search, float pruning_epsilon, float radius, uint32_t distinct, uint64_t* out_ids,
                         float* out_scores, uint32_t* out_counts, uint32_t* out_list_ids, uint32_t* out_list_counts);
/* The same on device pointers under the conventions of rbq_mstg_search_batch_device: enqueued on the caller's stream without
 * host synchronisation, one workspace per (index, stream). */
int rbq_mstg_range_batch_device(const rbq_index* idx, const float* d_queries, uint64_t nq, uint32_t query_dim, uint32_t capacity,
                                uint32_t ef_search, float pruning_epsilon, float radius, uint32_t distinct, uint64_t* d_out_ids,
                                float* d_out_scores, uint32_t* d_out_counts, uint32_t* d_out_list_ids,
                                uint32_t* d_out_list_counts, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* RBQ_MSTG_RANGE_H */
