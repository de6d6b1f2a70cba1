/*
 * rbq_bf_range.h — C ABI of the range search on brute-force handles: every vector of the index whose
 * distance to a query is below a radius.  The brute-force index evaluates every vector for every query, so the answer loses
 * nothing to probing.  No counterpart in lqhl/rabitq-rs.  A header of its own under include/ext/, included as
 * "ext/rbq_bf_range.h": rbq_bf.h and the set of headers in include/ itself stay as they are.  The entry is exported by the
 * same library.
 */
#ifndef RBQ_BF_RANGE_H
#define RBQ_BF_RANGE_H

#include <stdint.h>

#include "../rbq_bf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Range search over the distances rbq_bf_search_batch ranks (search_internal's, bit for bit).  Per query:
 *  1. A vector matches iff its distance d is finite and d < radius, for both metrics: `radius` is a threshold on the distance,
 *     which for inner product is minus the score.  A vector the filter leaves out never matches (filter_words / filter_nbits as
 *     for rbq_bf_search_batch).  +inf matches every finite distance, -inf nothing; a NaN radius is RBQ_INVALID_CONFIG.
 *  2. The matches come back in ascending id order.  out_scores holds d (L2) or -d (inner product), as rbq_bf_search_batch
 *     reports it.  out_counts[q] is the total and may exceed `capacity` — that is how a short row shows; the first
 *     min(total, capacity) matches are written, the other slots of the row are UINT64_MAX / NaN.  The same call gives the same
 *     bytes every time.
 *  3. capacity == 0 counts only: out_ids and out_scores may be NULL.  A capacity above the index's length is legal; the rows
 *     keep the stride `capacity`.
 *   queries [nq][query_dim] host f32; out_ids [nq][capacity] u64, out_scores [nq][capacity] f32, out_counts [nq] u32, host.
 * Errors in the search's order: a null index, then EMPTY_INDEX, then DIMENSION_MISMATCH; then nq == 0 returns RBQ_OK; then
 * RBQ_INVALID_CONFIG for nq >= 2^31, a null `queries` or `out_counts`, null rows with capacity > 0, and a NaN radius — all
 * before the first HIP call.  Re-entrant on one handle (each call has a stream and a workspace of its own; the batch is cut into
 * sub-batches of queries and chunks of vectors, and the result does not depend on the cut).  Never aborts: device failures are
 * RBQ_DEVICE. */
int rbq_bf_range_batch(const rbq_bf_index* idx, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t capacity,
                       float radius, const uint32_t* filter_words, uint64_t filter_nbits, uint64_t* out_ids, float* out_scores,
                       uint32_t* out_counts);
/* The handle's metric (RBQ_METRIC_L2 / RBQ_METRIC_IP; a null handle: RBQ_METRIC_L2): what a caller that thinks in scores
 * needs to turn "score > s" into the distance threshold -s above. */
uint32_t rbq_bf_metric(const rbq_bf_index* idx);

#ifdef __cplusplus
}
#endif

#endif /* RBQ_BF_RANGE_H */
