/*
 * rbq_bf_range.h — C ABI of the range search on brute-force handles: every vector of the index whose
 * distance to a query is below a radius.  The brute-force index evaluates every vector for every query, so the answer loses
 * nothing to probing.  No counterpart in lqhl/rabitq-rs.  A header of its own under include/ext/, included as
 * "ext/rbq_bf_range.h": rbq_bf.h and the set of headers in include/ itself stay as they are.  The entry is exported by the
 * same library.  The raw rows attached here also serve the exact top-k search at the end of this header.
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

/* ---- exact range search against attached raw vectors ----------------------------------------------------
 * Raw rows for rbq_bf_range_exact_batch: `vectors` is [n][dim] elements of raw_dtype (RBQ_RAW_F32, RBQ_RAW_F16 or RBQ_RAW_BF16 of
 * rbq.h), row i the vector of id i — a brute-force index has no id array, an id is a position.  Host memory is copied to the
 * handle's device; a device pointer on that device is BORROWED: it stays the caller's and must outlive the attachment (memory is
 * told apart as rbq_bf_train_device tells it).  The library never rounds: a 16-bit element is widened exactly where a kernel loads
 * it.  NULL detaches (n and raw_dtype are then ignored).
 * RBQ_INVALID_CONFIG with the detail set, the handle keeping what it had: a null index; an unknown raw_dtype; n != rbq_bf_len(idx)
 * (these before the first HIP call); a borrowed pointer to 16-bit rows that is not 2-byte aligned.
 * The handles rbq_bf_append and rbq_bf_remove_ids return carry no raw rows, and RBF1 neither stores nor loads them.
 * NOT safe concurrently with any other call on the same handle: the old rows are released here. */
int rbq_bf_set_rerank_vectors(rbq_bf_index* idx, const void* vectors, uint64_t n, int raw_dtype);
/* RBQ_RAW_* of the attached rows; -1 with none attached, or for a null handle. */
int rbq_bf_rerank_dtype(const rbq_bf_index* idx);

/* Range search decided by the raw rows.  Per query:
 *  1. The candidates are exactly the matches of rbq_bf_range_batch at radius = candidate_radius: the estimate is finite and
 *     < candidate_radius and the filter lets the vector through.  +inf makes every such vector a candidate: a flat exact range
 *     search.
 *  2. Every candidate is scored against raw row [id] by the canonical sums (l2_distance_sqr / dot of src/math.rs, bit for bit):
 *     d = l2_distance_sqr (L2) or -dot (inner product).  It matches iff d is finite and d < x — one rule on the distance for both
 *     metrics, as in rbq_bf_range_batch.
 *  3. Rows and counts as rbq_bf_range_batch writes them: matches in ascending id order, out_scores = d (L2) or -d (inner product),
 *     out_counts[q] the total (it may exceed `capacity`), unused slots UINT64_MAX / NaN, capacity == 0 counts only (the rows may be
 *     NULL), a capacity above the index's length is legal.  The same call gives the same bytes every time.
 * Errors, all before the first HIP call: those of rbq_bf_range_batch up to nq == 0 (RBQ_OK) in its order; then RBQ_INVALID_CONFIG
 * with the detail set when no raw vectors are attached — nothing is silently approximated; then the remaining checks of
 * rbq_bf_range_batch, a NaN `x` and a NaN `candidate_radius` refused.  Re-entrant on one handle like rbq_bf_range_batch (but not
 * with rbq_bf_set_rerank_vectors).  Never aborts: device failures are RBQ_DEVICE. */
int rbq_bf_range_exact_batch(const rbq_bf_index* idx, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t capacity, float x,
                             float candidate_radius, const uint32_t* filter_words, uint64_t filter_nbits, uint64_t* out_ids,
                             float* out_scores, uint32_t* out_counts);

/* ---- exact top-k search against the attached raw vectors ------------------------------------------------
 * The nearest neighbours decided by the raw rows.  Per query, with P = max(pool, top_k) <= 4096:
 *  1. The candidate pool is exactly what rbq_bf_search_batch returns at top_k := P with the same filter: the best P estimates with
 *     the crate's heap and its ties, fewer where the filter or the index leaves fewer.
 *  2. Every pool entry is scored against raw row [id] by the canonical sums (l2_distance_sqr / dot of src/math.rs, bit for bit):
 *     d = l2_distance_sqr (L2) or -dot (inner product).  An entry whose d is not finite is dropped.
 *  3. The survivors are ordered by d ascending (-0.0 and +0.0 are one value), then by id ascending; the first top_k are written:
 *     out_scores holds d (L2) or -d (inner product), unused slots are UINT64_MAX / NaN, out_counts[q] = min(top_k, survivors).
 *     The same call gives the same bytes every time.
 *   queries [nq][query_dim] host f32; out_ids [nq][top_k] u64, out_scores [nq][top_k] f32, out_counts [nq] u32, host.
 * Errors, all before the first HIP call: those of rbq_bf_search_batch up to nq == 0 (RBQ_OK) in its order; top_k == 0 zeroes the
 * counts and returns RBQ_OK; then RBQ_INVALID_CONFIG with the detail set when no raw vectors are attached — nothing is silently
 * approximated —, for P > 4096, for nq >= 2^31 and for a null buffer.  Re-entrant on one handle like rbq_bf_search_batch (but not
 * with rbq_bf_set_rerank_vectors).  Never aborts: device failures are RBQ_DEVICE. */
int rbq_bf_search_exact_batch(const rbq_bf_index* idx, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t top_k,
                              uint32_t pool, const uint32_t* filter_words, uint64_t filter_nbits, uint64_t* out_ids, float* out_scores,
                              uint32_t* out_counts);

/* ---- the same search with the pool chosen by rank --------------------------------------------------------
 * rbq_bf_search_exact_batch with another rule for step 1, for callers that want the exact neighbours and not the crate's tie
 * behaviour inside the pool:
 *  1. The candidates are the vectors the filter lets through whose estimate d — the distance rbq_bf_search_batch ranks, bit for
 *     bit — is finite.  The pool is the first min(P, candidates) of them by the key (f32::total_cmp order of d, id ascending):
 *     the heap's comparison, but among EQUAL estimates at the pool's boundary the smallest ids win.  A radix select over the
 *     distances finds it, no heap: rbq_bf_debug_select_launches() and the handle's heap statistics do not move.
 *  2, 3. As above; the same call gives the same bytes every time, whatever the cut into sub-batches and chunks.
 * Parameters, buffers, errors (their order and texts) and re-entrancy are those of rbq_bf_search_exact_batch. */
int rbq_bf_search_exact_ranked_batch(const rbq_bf_index* idx, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t top_k,
                                     uint32_t pool, const uint32_t* filter_words, uint64_t filter_nbits, uint64_t* out_ids,
                                     float* out_scores, uint32_t* out_counts);

#ifdef __cplusplus
}
#endif

#endif /* RBQ_BF_RANGE_H */
