/*
 * rbq_mstg.h — C ABI of the MSTG posting-list build: steps 2 and 3 of lqhl/rabitq-rs's `MstgIndex::build`
 * (reference src/mstg/index.rs:40-110) on the device.  Closure assignment (ClosureAssigner::assign,
 * src/mstg/closure.rs:24-107) decides which lists hold each vector; the encoder of rbq_index_build_device_ex then
 * quantises every (vector, list) pair against the list's centroid in the raw space (PostingList::quantize_vectors,
 * src/mstg/posting_list.rs:66-101).  The result is an ordinary rbq_index with rotator RBQ_ROTATOR_NONE, served by
 * rbq_posting_scan_batch, and by rbq_mstg_search_batch below, which answers `MstgIndex::search` / `batch_search`
 * (src/mstg/index.rs:149-213, 340-346) in one call: the centroid ranking and dynamic_prune run on the device too.
 * Step 1, the hierarchical balanced clustering that yields the centroids (HierarchicalClustering::cluster,
 * src/mstg/clustering.rs), is rbq_mstg_cluster_device.  Step 4 (HNSW over the centroids) is not built: it is not needed for
 * searching through this library.  A header of its own, not included by rbq.h (DESIGN.md sections 15, 16, 17).  Saving and
 * loading the result in the crate's `.mstg` format: rbq_mstg_persist.h (section 18).  Appending rows to the result and removing
 * ids from it without a rebuild: rbq_mstg_mutate.h (section 24).
 */
#ifndef RBQ_MSTG_H
#define RBQ_MSTG_H

#include <stddef.h>
#include <stdint.h>

#include "rbq.h"
#include "rbq_mstg_persist.h" /* rbq_mstg_save* / rbq_mstg_load*: the crate's `.mstg` file */
#include "rbq_mstg_mutate.h"  /* rbq_mstg_append / rbq_mstg_remove_ids: add and remove_ids on the GPU */

#ifdef __cplusplus
extern "C" {
#endif

#define RBQ_MSTG_MAX_REPLICAS 64   /* largest max_replicas served (the crate's default is 8) */
#define RBQ_MSTG_SHORTLIST    256  /* entries per row of rbq_mstg_debug_closure_shortlist */

/* ClosureAssigner{epsilon, max_replicas}.assign(row, centroids) for every row of `data`, bit for bit: distances are
 * math::l2_distance_sqr in the order an AVX2 host takes (8 accumulators, src/math.rs:216-245), the sort is stable (equal
 * distances keep ascending centroid index), the threshold is closest * (1.0f + epsilon) with the sum rounded first, and
 * the RNG rule compares with a strict >.  The result equals rbq_build_closure_assign of the CPU builder.
 *   centroids  [n_lists][dim] f32, host or device memory (detected)
 *   data       [n][dim] f32, host or device memory (detected; host rows are copied a chunk at a time).  Any dim >= 1.
 *   max_chunk_rows  upper bound on the rows per pass; 0 = as many as a 512 MiB workspace holds.  The result does not
 *              depend on it.
 *   device     HIP ordinal, -1 = the current device
 *   out_lists  [n][max_replicas] u32, host or device memory (detected): row i holds the crate's Vec for vector i in its
 *              order (closest list first); unused slots are UINT32_MAX.   out_counts [n] u32: the Vec's length (>= 1).
 * Errors, all checked before the first HIP call: RBQ_INVALID_CONFIG for a null pointer, n == 0, n_lists == 0 or
 * >= 2^32 - 1, dim == 0, n >= 2^32 - 16, max_replicas == 0 or > RBQ_MSTG_MAX_REPLICAS, epsilon negative or not finite
 * (the crate panics on max_replicas == 0 and on a NaN distance).  A non-finite value in data or centroids is
 * RBQ_INVALID_CONFIG too: it is found on the device, chunk by chunk, before the chunk is scored, so the rows of earlier
 * chunks have been written by then.  After any error the contents of the outputs are unspecified.  Never aborts: device
 * failures are RBQ_DEVICE. */
int rbq_mstg_closure_assign(const float* centroids, uint64_t n_lists, uint32_t dim, const float* data, uint64_t n,
                            float epsilon, uint32_t max_replicas, uint64_t max_chunk_rows, int device,
                            uint32_t* out_lists, uint32_t* out_counts);

/* MstgIndex::build steps 2 and 3: closure assignment of every row, then the posting lists.  List c holds the vectors
 * assigned to it in ascending vector index (src/mstg/index.rs:61-66); a vector may sit in several lists; ids are the
 * row indices.  The index equals, array for array, rbq_index_create_with_recon over the CPU builder's
 * train_with_clusters fed the expanded (vector, list) pairs sorted by (list, vector).
 *   hdr        dim, padded_dim == dim (a multiple of 16), metric, rotator RBQ_ROTATOR_NONE without blob, ex_bits,
 *              n_lists = number of centroids; n_vectors is ignored
 *   centroids  [n_lists][dim], data [n][dim]: host or device memory (detected).  Host data is uploaded whole: the
 *              encoder gathers rows by list.
 *   rescale    RBQ_RESCALE_CONST (t_const > 0 when ex_bits > 0: what PostingList::quantize_vectors derives with seed
 *              42) or RBQ_RESCALE_OPTIMAL, as for rbq_index_build_device_ex
 *   max_chunk_rows  as above; the result does not depend on it
 * Errors as for rbq_mstg_closure_assign, plus a header that validate fails or whose rotator is not RBQ_ROTATOR_NONE,
 * an unknown rescale mode and a missing t_const; all before the first HIP call.  One device only. */
int rbq_mstg_build_device(const rbq_header* hdr, const float* centroids, const float* data, uint64_t n,
                          float closure_epsilon, uint32_t max_replicas, int rescale, float t_const,
                          uint64_t max_chunk_rows, int device, rbq_index** out);

/* MstgIndex::build step 1: HierarchicalClustering{max_posting_size, branching_factor, balance_weight, max_iterations}
 * .cluster(data) on the device.  The crate's own result cannot be reproduced (its k-means merges sums in thread order and
 * its RNG is ChaCha12); the specification is the CPU restatement rbq_build_hcluster of the CPU builder, whose pins
 * csrc/host/rbq_hcluster.hpp states, and every array of the result equals it bit for bit.
 *   data       [n][dim] f32, host or device memory (detected; host data is uploaded once).  Any dim >= 1.
 *   max_posting_size  a cluster of at most this many rows is final (MstgConfig::max_posting_size)
 *   branching_factor  k of every split's k-means; up to 256 a direct assignment kernel runs, above it the GEMM shortlist of
 *              rbq_kmeans_device
 *   balance_weight    any value: NaN or <= 0 means no balancing, +inf that no subcluster is ever oversized
 *   max_iterations    Lloyd iterations per split (the crate: 100)
 *   host_below a cluster of at most this many rows is clustered on the host together with its whole subtree (small splits
 *              are bound by launch latency).  0 = never; RBQ_MSTG_HOST_BELOW_DEFAULT = the library's choice
 *              (RBQ_MSTG_HOST_BELOW).  The result does not depend on it.
 *   device     HIP ordinal, -1 = the current device
 *   out        a handle read through the accessors below and released with rbq_hclustered_free: the final clusters in
 *              the crate's pop order; centroids [count][dim]; offsets [count + 1]; members [n] u32, the row indices cluster
 *              by cluster, each cluster in its own order; stats [6]: splits, balance moves, empty clusters reseeded,
 *              reseeds drawn from the RNG, splits that ran on the host, bytes of device workspace.
 * RBQ_INVALID_CONFIG, checked before the first HIP call: a null pointer, n == 0, dim == 0, n >= 2^32 - 1,
 * max_iterations == 0, branching_factor < 2 (the crate panics on 0 and never ends with 1) or > max_posting_size + 1 (a
 * cluster one row over the limit has fewer rows than centroids: the crate panics).  Found later: a non-finite value
 * (on the device, before any split), and a split that leaves a single non-empty subcluster, on which the crate would
 * loop for ever (identical rows without balancing).  One device.  Never aborts: device failures are RBQ_DEVICE. */
#define RBQ_MSTG_HOST_BELOW_DEFAULT UINT64_MAX
#define RBQ_MSTG_HOST_BELOW 0 /* not measured yet: every split runs on the device */
typedef struct rbq_hclustered rbq_hclustered;
int rbq_mstg_cluster_device(const float* data, uint64_t n, uint32_t dim, uint64_t max_posting_size, uint64_t branching_factor,
                            float balance_weight, uint64_t max_iterations, uint64_t host_below, int device,
                            rbq_hclustered** out);
uint64_t        rbq_hclustered_count(const rbq_hclustered* h);
const float*    rbq_hclustered_centroids(const rbq_hclustered* h);
const uint64_t* rbq_hclustered_offsets(const rbq_hclustered* h);
const uint32_t* rbq_hclustered_members(const rbq_hclustered* h);
const uint64_t* rbq_hclustered_stats(const rbq_hclustered* h);
void            rbq_hclustered_free(rbq_hclustered* h);

/* Diagnostic: rows, summed over every closure assignment of this process, whose shortlist could not be proven complete
 * within RBQ_MSTG_SHORTLIST entries and that were scored exactly against every centroid instead. */
uint64_t rbq_mstg_debug_closure_fallbacks(void);
/* Diagnostic tap: the shortlist of every row as the closure assignment forms it, nothing else computed.  out_sl
 * [n][RBQ_MSTG_SHORTLIST] u32 centroid indices ascending, out_sl_n [n] their number, or UINT32_MAX for a row that
 * falls back to every centroid.  With n_lists <= RBQ_MSTG_SHORTLIST no shortlist is formed: every row lists all
 * centroids.  Host outputs; arguments and errors as for rbq_mstg_closure_assign. */
int rbq_mstg_debug_closure_shortlist(const float* centroids, uint64_t n_lists, uint32_t dim, const float* data, uint64_t n,
                                     uint32_t max_replicas, uint64_t max_chunk_rows, int device, uint32_t* out_sl,
                                     uint32_t* out_sl_n);

/* MstgIndex::search for every query, in one call: the centroid search, dynamic_prune and the posting-list scan.
 *
 * The selection.  The crate's candidate lists come from an HNSW built by parallel_insert: approximate, and different
 * from run to run.  This call returns what that HNSW approximates, the exact ef_search nearest centroids.  Per query:
 *  1. S(c) = math::l2_distance_sqr(query, centroid c) in the AVX2 order, the value rbq_posting_scan_batch takes g_add
 *     from.  L2 for both metrics, as the crate's centroid index (DistL2, src/mstg/hnsw.rs:91-97), on the full-precision
 *     centroids of the handle.
 *  2. The centroids are ordered by (bit pattern of S, centroid index) ascending and the first
 *     ef = min(ef_search, n_lists) are kept.  This refines the crate's order by sqrtf(S): where two different S round
 *     to one square root the HNSW's order is unspecified anyway.
 *  3. d(c) = sqrtf(S(c)) correctly rounded, thr = d(first) * (1.0f + pruning_epsilon) in f32 with the sum rounded
 *     first (dynamic_prune, src/mstg/index.rs:349-362); a candidate is kept while d(c) <= thr, which is a prefix.
 *     No pruning_epsilon is rejected: a negative one can prune even the closest list and NaN prunes every list, as
 *     the crate's comparison does.  The one deliberate rule: when any S(c) of a query is NaN, or its smallest S is
 *     +inf, nothing is selected (the HNSW's behaviour there is undefined).
 *  4. The kept lists are scanned in that order exactly as rbq_posting_scan_batch scans a caller's lists: binary
 *     estimate only, g_add = S (L2) or the canonical -dot (inner product), non-finite estimates dropped, L2 estimates
 *     clamped to >= 0, the smallest top_k kept, the earlier candidate in (list order, vector order) winning a tie;
 *     distances are reported for both metrics.
 *  5. ef_search == 0 or top_k == 0: RBQ_OK with every count 0.  Empty lists contribute nothing.
 * The result equals rbq_build_mstg_select_lists of the CPU builder followed by rbq_posting_scan_batch, bit for bit.
 *
 *   queries     [nq][query_dim] f32, host memory; cut into chunks that keep the work list and the score matrix inside
 *               a fixed workspace (1 GiB); the result does not depend on the chunking
 *   out_ids     [nq][top_k] u64, out_scores [nq][top_k] f32 ascending, out_counts [nq] u32; unused slots are
 *               UINT64_MAX / NaN
 *   out_list_ids [nq][min(ef_search, n_lists)] u32: the selected lists in scan order, unused slots UINT32_MAX;
 *   out_list_counts [nq] u32: how many.  Either may be NULL.
 * Every ef_search and every n_lists the handle can hold is served.  Handles of up to RBQ_MSTG_SHORTLIST lists score
 * every centroid exactly; larger ones take a GEMM shortlist that is rescored exactly, and a query
 * whose shortlist cannot be proven complete within RBQ_MSTG_SEARCH_SHORTLIST entries is scored against every centroid
 * and counted (rbq_mstg_debug_search_fallbacks), never approximated.
 * Errors, all checked before the first HIP call, in this order: a null index; RBQ_EMPTY_INDEX; RBQ_DIMENSION_MISMATCH;
 * RBQ_INVALID_CONFIG for an index whose rotator is not RBQ_ROTATOR_NONE; (nq == 0 is RBQ_OK;) RBQ_INVALID_CONFIG for a
 * null queries / out_counts, a null out_ids / out_scores unless top_k == 0 (they then hold no element), or
 * top_k > 2^20.  One device: the first replica serves the call. */
#define RBQ_MSTG_SEARCH_SHORTLIST 2048
int rbq_mstg_search_batch(const rbq_index* idx, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t top_k,
                          uint32_t ef_search, float pruning_epsilon, uint64_t* out_ids, float* out_scores,
                          uint32_t* out_counts, uint32_t* out_list_ids, uint32_t* out_list_counts);

/* The same on device pointers, enqueued on the caller's stream without host synchronisation, under the conventions of
 * rbq_search_batch_device: one workspace per (index, stream), released by rbq_release_stream; calls on one stream are
 * stream-ordered.  The first call on a handle of more than RBQ_MSTG_SHORTLIST lists prepares the centroid images and
 * waits for them once.  d_out_list_ids / d_out_list_counts may be NULL. */
int rbq_mstg_search_batch_device(const rbq_index* idx, const float* d_queries, uint64_t nq, uint32_t query_dim,
                                 uint32_t top_k, uint32_t ef_search, float pruning_epsilon, uint64_t* d_out_ids,
                                 float* d_out_scores, uint32_t* d_out_counts, uint32_t* d_out_list_ids,
                                 uint32_t* d_out_list_counts, void* hip_stream);

/* The refined search: opt-in, a pure function of what rbq_mstg_search_batch returns.  The crate's MSTG
 * search ranks by the 1-bit estimate only and may return one id several times (closure assignment puts a vector into up to
 * max_replicas lists); this call re-scores a pool of binary candidates with the stored ex codes and returns distinct ids.
 * Per query, with pool = max(refine_pool, top_k):
 *  1. The pool is the result of rbq_mstg_search_batch with top_k := pool: same lists, list order, estimate, clamp, drop of
 *     non-finite estimates and tie rule.  Entry r of it is the candidate of rank r, a (list, position) entry: two ranks may carry
 *     one id.  out_list_ids / out_list_counts are that call's.
 *  2. The refined distance of a candidate is the crate's IVF refinement (src/ivf.rs:2086-2099): with ip the candidate's binary
 *     ip_x0_qr, t = binary_scale * ip; t += ex_dot; t += kbx_sum_q; dist = (f_add_ex + g_add) + f_rescale_ex * t, g_add the
 *     value the binary stage used for the candidate's list, ex_dot in the handle's numeric variant
 *     (rbq_index_set_numeric_variant: all three are served).  With ex_bits == 0 it is the binary estimate.  A non-finite
 *     refined distance drops the candidate; an L2 distance below zero is reported as zero; distances are reported for both metrics.
 *  3. Among the candidates with one id the smallest refined distance is kept, on equal values the smaller rank.
 *  4. The kept candidates are ordered by (refined distance by value, rank) ascending and the first top_k are returned:
 *     out_counts their number, unused slots UINT64_MAX / NaN.
 *  5. top_k == 0 or ef_search == 0: RBQ_OK with every count 0; nq == 0: RBQ_OK.
 * Errors: those of rbq_mstg_search_batch in its order, then RBQ_INVALID_CONFIG for pool > RBQ_MSTG_REFINE_POOL_MAX (one
 * workgroup sorts a query's pool in LDS); all before the first HIP call.  The result does not depend on the chunking (the pool's
 * slots, estimates and counts are part of the 1 GiB workspace).  The first refined call on a handle builds an identity slot map
 * (8 bytes per slot, through which the unchanged scan kernels report positions) and waits for it once.
 *
 * Exact rerank of the pool: with rbq_debug_set_option(idx, "mstg_rerank", 1) (every replica, default 0, any
 * non-zero value stores 1, with or without vectors attached) the two refined entries, and only they, replace steps 2 to 4:
 *  2'. Among the pool's entries with one id the one of the smallest rank stays (the exact score depends on the id alone, so every
 *      distinct id's raw row is read once per query).  The id of an entry is the stored id of its (list, position).
 *  3'. The distance of an entry is exact: the bits of the canonical l2_distance_sqr (L2) or of minus the canonical dot (inner
 *      product: a distance, with the sign of the MSTG estimate) between the caller's query row, widened as "query_dtype" says, and
 *      row `id` of the vectors attached with rbq_index_set_rerank_vectors (f32, f16 or bf16 rows).  An entry whose id is >= n, or
 *      whose exact distance is not finite, is dropped.  The stored ex codes are not read and the numeric variant does not enter.
 *  4'. The entries are ordered by (distance by value, -0.0 equal to +0.0; then rank) and the first top_k are returned as in step 4.
 * Step 1, step 5 and the list outputs are unchanged.  Errors: the refined call's, then RBQ_INVALID_CONFIG (detail set) if the
 * replica that serves the call has no raw vectors attached or its "rerank" is 0 — nothing is silently approximated; the check
 * comes before any kernel launch and also refuses a call with top_k == 0 or ef_search == 0.  With the option 0 a refined call never
 * looks at attached vectors.  rbq_mstg_search_batch*, rbq_posting_scan_batch and the IVF entry points never read the option. */
#define RBQ_MSTG_REFINE_POOL_MAX 4096
int rbq_mstg_search_refined_batch(const rbq_index* idx, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t top_k,
                                  uint32_t ef_search, float pruning_epsilon, uint32_t refine_pool, uint64_t* out_ids,
                                  float* out_scores, uint32_t* out_counts, uint32_t* out_list_ids, uint32_t* out_list_counts);
/* The same on device pointers under the conventions of rbq_mstg_search_batch_device: enqueued on the caller's stream without
 * host synchronisation (but for the one-time preparations), one workspace per (index, stream). */
int rbq_mstg_search_refined_batch_device(const rbq_index* idx, const float* d_queries, uint64_t nq, uint32_t query_dim,
                                         uint32_t top_k, uint32_t ef_search, float pruning_epsilon, uint32_t refine_pool,
                                         uint64_t* d_out_ids, float* d_out_scores, uint32_t* d_out_counts,
                                         uint32_t* d_out_list_ids, uint32_t* d_out_list_counts, void* hip_stream);

/* Diagnostic: queries, summed over every MSTG search of this process, that were scored against every centroid because
 * their shortlist could not be proven complete.  Waits for the devices' work. */
uint64_t rbq_mstg_debug_search_fallbacks(void);

#ifdef __cplusplus
}
#endif

#endif /* RBQ_MSTG_H */
