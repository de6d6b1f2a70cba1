/*
 * rbq.h — C ABI of the MI355X-native IVF+RaBitQ candidate-scan engine.
 *
 * This is the drop-in boundary for ONE path of lqhl/rabitq-rs: the query-time
 * scan `IvfRabitqIndex::search` / `batch_search` / `search_filtered`
 * (reference src/ivf.rs:1705-1752) whose body is `search_fastscan`
 * (src/ivf.rs:1754-1895) + `search_cluster_v2_batched` (src/ivf.rs:1901-2129).
 * Everything from `rotator.rotate(query)` to the sorted result vector runs on
 * the GPU behind `rbq_search_batch`.  Index training stays with the caller.
 *
 * The reference has no FFI seam of its own (search_fastscan is a private
 * method over private fields, src/ivf.rs:935-946), so the boundary is cut at
 * the two places a maintainer can reach without touching the algorithm:
 *   - the in-memory `ClusterData` arrays (src/ivf.rs:205-242) -> rbq_index_create
 *   - the persisted RBQ1-v3 byte stream (src/ivf.rs:1317-1474) -> rbq_index_load_rbq1
 * INTEGRATION.md shows the Rust-side `extern "C"` binding for both.
 *
 * Plain pointers and sizes only; no torch / HIP types in any signature.
 */
#ifndef RBQ_H
#define RBQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes: 1:1 with `RabitqError` (reference src/lib.rs:39-57) ---- */
#define RBQ_OK                   0
#define RBQ_DIMENSION_MISMATCH   1 /* RabitqError::DimensionMismatch{expected,got} */
#define RBQ_INVALID_CONFIG       2 /* RabitqError::InvalidConfig(msg)             */
#define RBQ_EMPTY_INDEX          3 /* RabitqError::EmptyIndex                     */
#define RBQ_IO                   4 /* RabitqError::Io                             */
#define RBQ_INVALID_PERSISTENCE  5 /* RabitqError::InvalidPersistence(msg)        */
#define RBQ_DEVICE               6 /* hipError_t / launch failure (new: no CPU fallback exists) */

#define RBQ_METRIC_L2 0            /* metric_to_tag, src/ivf.rs:122-127 */
#define RBQ_METRIC_IP 1
#define RBQ_ROTATOR_MATRIX 0       /* RotatorType, src/rotation.rs:10-15 */
#define RBQ_ROTATOR_FHT_KAC 1
#define RBQ_ROTATOR_NONE 2         /* no query-time rotation: MSTG posting lists (src/mstg/posting_list.rs:66-101)
                                      are quantised on raw residuals; padded_dim == dim, rotator_len == 0.
                                      Not a tag of the RBQ1 format (rbq_index_load_rbq1 rejects it). */

/* FASTSCAN_BATCH_SIZE, src/simd.rs:768 */
#define RBQ_BATCH 32

typedef struct rbq_index rbq_index;     /* opaque; owns device memory on one or N GPUs (replicas of one index) */
typedef struct rbq_builder rbq_builder; /* opaque; an index under construction by the streamed GPU encoder   */

/* Mirrors the scalar fields of `IvfRabitqIndex` (src/ivf.rs:935-946) and the
 * RBQ1-v3 header (src/ivf.rs:1324-1373). */
typedef struct {
    uint32_t dim;          /* query dimensionality                                  */
    uint32_t padded_dim;   /* rotator.padded_dim(): dim rounded up to x64 for FhtKac */
    uint8_t  metric;       /* RBQ_METRIC_*                                          */
    uint8_t  rotator;      /* RBQ_ROTATOR_*                                         */
    uint8_t  ex_bits;      /* total_bits-1; only 0, 2, 6 (src/simd.rs:3205-3215)    */
    uint8_t  reserved;
    uint64_t n_vectors;    /* sum of list sizes                                     */
    uint64_t n_lists;      /* clusters.len()                                        */
    const uint8_t* rotator_blob; /* DynamicRotator::serialize(): FhtKac = 4*D/8 flip
                                    bytes (src/rotation.rs:486-489); Matrix = D*D f32 LE */
    uint64_t rotator_len;
} rbq_header;

/* One `ClusterData` (src/ivf.rs:205-242), borrowed for the duration of the call. */
typedef struct {
    const float*    centroid;     /* [padded_dim], rotated space                     */
    uint64_t        n;            /* num_vectors                                     */
    const uint64_t* ids;          /* [n]                                             */
    const uint8_t*  batch_data;   /* exactly ClusterData.batch_data: ceil(n/32) records
                                     of [D*4 B FastScan codes | f_add[32] | f_rescale[32]
                                     | f_error[32]] (src/ivf.rs:247-316)             */
    uint64_t        batch_len;    /* ceil(n/32) * (D*4 + 384)                        */
    const uint8_t*  ex_codes;     /* [n][D*ex_bits/8] flattened ex_codes_packed; may be
                                     NULL when ex_bits == 0                          */
    const float*    f_add_ex;     /* [n] (ignored when ex_bits == 0)                 */
    const float*    f_rescale_ex; /* [n]                                             */
} rbq_list_view;

/* `SearchDiagnostics` (src/ivf.rs:150-155), one per query. */
typedef struct {
    uint64_t estimated;
    uint64_t skipped_by_lower_bound;
    uint64_t extended_evaluations;
} rbq_diag;

/* Build a device-resident index from ClusterData-shaped host arrays.  The reference bytes are uploaded as they
 * are and re-laid into the device layout by the GPU.
 * n_devices >= 1 replicas: devices[i] = HIP device ordinal of replica i (NULL = the current device for one
 * replica, devices 0..n-1 otherwise; an ordinal may repeat).  Replica 0 is built from the host arrays, the others
 * are device-to-device copies of it.  `rbq_search_batch` shards a batch over the replicas (the reference's
 * batch_search is a par_iter over queries, src/ivf.rs:1743-1752).  Inputs are copied; nothing is retained.
 * Test status: several replicas on ONE device (a repeated ordinal) are covered by the GPU suite; replicas on DISTINCT
 * devices (peer copy or pinned bounce, per-device launch state) have only run where tests/test_gpu_round3.py::
 * test_replicas_on_two_devices found two GPUs — the builder's boxes had one. */
int rbq_index_create(const rbq_header* hdr, const rbq_list_view* lists,
                     int n_devices, const int* devices, rbq_index** out);

/* Build a device-resident index straight from an RBQ1 v3 byte stream as
 * written by `IvfRabitqIndex::save_to_writer` (src/ivf.rs:1317-1474); applies
 * the same validation as `load_from_reader` (src/ivf.rs:1484-1702) incl. CRC32. */
int rbq_index_load_rbq1(const void* bytes, size_t len,
                        int n_devices, const int* devices, rbq_index** out);

/* GPU-side encoder: build the index on the device from raw vectors — the quantisation loop of
 * `IvfRabitqIndex::train_with_clusters` / `build_from_rotated` (src/ivf.rs:1025-1215: rotate, group by cluster in
 * ascending vector order, `quantize_with_centroid` src/quantizer.rs:140-262 with the constant rescale factor of
 * `RabitqConfig::faster`, src/quantizer.rs:33-46,563-592) — writing the device layout directly.  Clustering stays
 * with the caller (the reference accepts any clustering here).
 *   hdr        dim, padded_dim, metric, rotator (+ rotator_blob/len), ex_bits, n_lists; n_vectors is ignored
 *   centroids  HOST  [n_lists][dim]  cluster centroids in the input space
 *   d_data     DEVICE [n][dim]       vectors; the id of vector i is i
 *   d_assign   DEVICE [n]            cluster of every vector (< n_lists, else RBQ_INVALID_CONFIG)
 *   t_const    the constant scaling factor (`compute_const_scaling_factor`); required when ex_bits > 0
 * The result is identical, array for array, to rbq_index_create over the CPU path's ClusterData. */
int rbq_index_build_device(const rbq_header* hdr, const float* centroids, const float* d_data, const uint32_t* d_assign,
                           uint64_t n, float t_const, int device, rbq_index** out);

/* rbq_index_build_device with the rescale factor chosen by `rescale`:
 *   RBQ_RESCALE_CONST    RabitqConfig::faster — t_const for every vector (exactly rbq_index_build_device)
 *   RBQ_RESCALE_OPTIMAL  RabitqConfig::new — every vector's own best_rescale_factor (src/quantizer.rs:337-427), searched
 *                        on the GPU; t_const is ignored.  The result is identical, array for array, to rbq_index_create
 *                        over train_with_clusters(..., use_faster_config = false).  Moot for 1-bit indexes (ex_bits 0).
 * Any other value is RBQ_INVALID_CONFIG. */
#define RBQ_RESCALE_CONST   0  /* RabitqConfig::faster: t_const for every vector (t_const > 0 when ex_bits > 0) */
#define RBQ_RESCALE_OPTIMAL 1  /* RabitqConfig::new: best_rescale_factor per vector; t_const ignored            */
int rbq_index_build_device_ex(const rbq_header* hdr, const float* centroids, const float* d_data, const uint32_t* d_assign,
                              uint64_t n, int rescale, float t_const, int device, rbq_index** out);

/* The same encoder fed chunk by chunk, for indexes whose raw vectors do not fit in HBM at once (100 M x 768 f32 =
 * 307 GB): `train_with_clusters` (src/ivf.rs:1025-1215) builds cluster by cluster and never needs all vectors
 * resident either.  Protocol:
 *   begin   hdr / centroids / t_const as for rbq_index_build_device; list_sizes HOST [n_lists] = number of vectors
 *           each cluster will receive (the caller's count pass over its assignment).  All device arrays of the
 *           index are allocated here.
 *   push    `count` vectors with ids first_id .. first_id+count-1 and their cluster ids.  vectors [count][dim] f32
 *           and assign [count] u32 may each be HOST or DEVICE pointers (detected).  Chunks must arrive in ascending
 *           id order (list membership order = ascending vector index, src/ivf.rs:1141-1149).  A list that receives
 *           more vectors than announced, or a cluster id >= n_lists, is RBQ_INVALID_CONFIG; after an error the builder
 *           can only be aborted.
 *   finish  requires every announced vector to have been pushed; returns the index (identical, array for array,
 *           to rbq_index_build_device over the same data), replicated on n_devices (devices[0] must be the
 *           builder's device; NULL / 1 = that device only) and frees the builder.
 *   abort   frees a builder that was not finished. */
int rbq_build_stream_begin(const rbq_header* hdr, const float* centroids, const uint32_t* list_sizes, float t_const,
                           int device, rbq_builder** out);
/* rbq_build_stream_begin with a rescale mode (RBQ_RESCALE_*, as for rbq_index_build_device_ex). */
int rbq_build_stream_begin_ex(const rbq_header* hdr, const float* centroids, const uint32_t* list_sizes, int rescale,
                              float t_const, int device, rbq_builder** out);
int rbq_build_stream_push(rbq_builder* b, const float* vectors, const uint32_t* assign, uint64_t first_id, uint64_t count);
int rbq_build_stream_finish(rbq_builder* b, int n_devices, const int* devices, rbq_index** out);
void rbq_build_stream_abort(rbq_builder* b);

void rbq_index_destroy(rbq_index* idx);

/* Accessors (IvfRabitqIndex::len / cluster_count, src/ivf.rs:1218-1230). */
uint64_t rbq_index_len(const rbq_index* idx);
uint64_t rbq_index_cluster_count(const rbq_index* idx);
uint32_t rbq_index_dim(const rbq_index* idx);
uint32_t rbq_index_padded_dim(const rbq_index* idx);
uint32_t rbq_index_device_count(const rbq_index* idx); /* number of replicas */

/* `batch_search` (src/ivf.rs:1743-1752); nq = 1 is `search` (:1705);
 * filter_words != NULL is `search_filtered` (:1723): a dense bitset over the
 * u32 id space, bit i set <=> RoaringBitmap::contains(i) (src/ivf.rs:2018-2022).
 *
 * queries:    [nq][query_dim] row-major host f32
 * out_ids:    [nq][top_k]  (unused slots = UINT64_MAX)
 * out_scores: [nq][top_k]  (unused slots = NaN); L2: distance asc, IP: score desc
 * out_counts: [nq]         number of valid results of each query (<= top_k)
 * diag:       NULL or [nq]
 *
 * Errors follow search_fastscan: EMPTY_INDEX is checked before
 * DIMENSION_MISMATCH (src/ivf.rs:1761-1769); top_k == 0 returns RBQ_OK with all
 * counts 0 (:1792-1794); nprobe is clamped to [1, n_lists] (:1791).
 * Every nprobe (clamped to n_lists) and every top_k <= 2^20 is served.  Fast paths: nprobe <= 8192 (MFMA shortlist with
 * its key window in LDS; above it the exact all-pairs ranking with the window in global memory), top_k <= 256 (top-k in
 * registers), top_k <= 16384 (exact heap in the LDS of one compute unit: one workgroup per CU from top_k ~ 7000; above it
 * the heap lives in global memory).  top_k > 2^20, or nq * top_k * 8 bytes of heap workspace > 8 GiB in one device call, is
 * RBQ_INVALID_CONFIG; nq < 2^31 per call of the device entry.
 * RANGE SEARCH (option "range_search" 1 with the radius r of "range_radius_bits", rbq_debug_set_option; also through
 * rbq_search_batch_device): top_k is read as the CAPACITY of a query's row (<= 2^20; no heap workspace, no 8 GiB rule).  A vector
 * of the probed lists matches iff the reference's loop (src/ivf.rs:2013-2127) with the constant r in the place of the running
 * k-th distance evaluates it and finds distance < r (L2) or score > r (inner product).  out_counts[q] is the TOTAL number of
 * matches and may exceed top_k: that is how a caller sees truncation.  The first min(total, top_k) matches in scan order (probe
 * order, then position inside the list; not sorted by score) are written, the other slots are UINT64_MAX / NaN.  diag counts as in
 * that loop and does not depend on top_k.  Errors and the top_k == 0 case are as above.
 * EXACT RANGE SEARCH (options "range_exact" 1 with the exact radius x of "range_exact_radius_bits", while "range_search" is 1, raw
 * vectors are attached with rbq_index_set_rerank_vectors and the option "rerank" is 1): the matches of the range search above at
 * its radius r — the same call with "range_exact" 0 and the rerank off, at unlimited capacity, in its scan order, with the filter,
 * numeric variant, "query_dtype" and diagnostic options acting as they do there — are only CANDIDATES.  r stays on the estimate's
 * scale and bounds the work; with r = +inf (L2) or -inf (inner product) every probed vector that the reference's loop evaluates to
 * a finite distance is a candidate.  Each candidate id is scored exactly as the rerank scores it (the canonical l2_distance_sqr /
 * dot of src/math.rs between the caller's unrotated query and raw row id, 16-bit query or row elements widened where they are
 * loaded, raw rows of any "rerank_raw_dtype"; id >= n_raw scores the NaN 0x7fc00000) and matches iff exact distance < x (L2) or
 * exact dot product > x (inner product); NaN never matches.  out_counts[q] is the total number of matches and may exceed top_k (the
 * capacity, <= 2^20); the first min(total, top_k) matches are written in scan order with their EXACT scores, the other slots are
 * UINT64_MAX / NaN; the same call gives the same rows every time.  diag is that of the candidate call and depends on neither x nor
 * top_k.  "rerank_pool" is not read in range mode; "range_exact" has no effect while "range_search" is 0.  RBQ_INVALID_CONFIG
 * (detail set): "range_search" 1 and "range_exact" 1 without raw vectors attached or with "rerank" 0 — nothing is silently
 * approximated — and "range_search" 1 with the rerank on and "range_exact" 0.
 * 16-BIT QUERIES (option "query_dtype" RBQ_RAW_F16 / RBQ_RAW_BF16, rbq_debug_set_option): `queries` is read as nq rows of
 * query_dim 16-bit elements, 2 * query_dim bytes apart, passed through the `const float*` parameter as they are; query_dim stays a
 * count of elements, every check keeps its order and its text.  An element is widened to f32 exactly where a kernel loads it (f16
 * by the IEEE conversion, subnormals included; bf16 is bits << 16); the library never rounds a query.  The pointer must be 2-byte
 * aligned, else RBQ_INVALID_CONFIG ("queries: pointer not aligned to its 16-bit elements") before any device call; rows of odd
 * query_dim are 2-byte aligned only, and served.  Contract: ids, counts, score bits, diag, list outputs and errors of a call with
 * 16-bit queries equal those of the same call with "query_dtype" RBQ_RAW_F32 on the rows widened to f32.  The option is state of
 * the handle: changing it while a call is in flight on that handle is the caller's problem.
 * Re-entrant on one handle.  The batch is cut into sub-batches that are pipelined over a few streams: host
 * staging and PCIe copies of one sub-batch overlap the kernels of the others.  Buffers that are page-locked
 * (rbq_host_alloc, hipHostMalloc, hipHostRegister) are DMA-ed directly; pageable ones are staged through the
 * handle's pinned buffers.  With N replicas the queries are split into N contiguous shards, one per device. */
int rbq_search_batch(const rbq_index* idx, const float* queries, uint64_t nq,
                     uint32_t query_dim, uint32_t top_k, uint32_t nprobe,
                     const uint32_t* filter_words, uint64_t filter_nbits,
                     uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                     rbq_diag* diag);

/* MSTG posting-list scan: the caller (MstgIndex::search, src/mstg/index.rs:149-213) has
 * already chosen the posting lists of each query (HNSW centroid search + dynamic pruning stay on the
 * CPU); this scans them like search_posting_list_fastscan (src/mstg/index.rs:216-330) — binary FastScan
 * estimate only, f_error/g_error = 0, non-finite estimates dropped, L2 estimates clamped to >= 0 — and
 * keeps the top_k smallest distances like the partial sort of MstgIndex::search (:185-205; ties there
 * are unordered, here the earlier candidate in (list order, vector order) wins).
 *
 * list_ids:    [nq][max_lists] posting-list (cluster) ids per query, scanned in the given order
 * list_counts: [nq]            number of valid entries of each row (<= max_lists)
 * out_*:       as rbq_search_batch; out_scores are distances (ascending) for both metrics
 * The index must have been created with rotator = RBQ_ROTATOR_NONE. */
int rbq_posting_scan_batch(const rbq_index* idx, const float* queries, uint64_t nq, uint32_t query_dim,
                           uint32_t top_k, const uint32_t* list_ids, const uint32_t* list_counts,
                           uint32_t max_lists, uint64_t* out_ids, float* out_scores, uint32_t* out_counts);



/* Same operation on DEVICE pointers (queries and outputs already in HBM of the index's device), ENQUEUED on
 * `hip_stream` (a hipStream_t passed as void*, NULL = default stream) and returning without host
 * synchronisation: results are valid once the stream reaches this point. Each stream gets its own scratch
 * workspace inside the handle; issue calls for one stream from one host thread at a time.
 * d_filter_words may be NULL. d_diag is NULL or [nq] rbq_diag in device memory.
 * A handle with several replicas serves the call from the replica on the device that owns d_queries. */
int rbq_search_batch_device(const rbq_index* idx, const float* d_queries, uint64_t nq,
                            uint32_t query_dim, uint32_t top_k, uint32_t nprobe,
                            const uint32_t* d_filter_words, uint64_t filter_nbits,
                            uint64_t* d_out_ids, float* d_out_scores,
                            uint32_t* d_out_counts, rbq_diag* d_diag,
                            void* hip_stream);

/* Frees the scratch workspace the handle keeps for `hip_stream` (rbq_search_batch_device creates one per caller
 * stream and keeps it until the index is destroyed); call it before destroying a stream that will not be used
 * with this index again.  The stream must be idle. */
int rbq_release_stream(rbq_index* idx, void* hip_stream);

/* IvfRabitqIndex::fetch_embedding (src/ivf.rs:1247-1307) for n ids.  out [n][dim] f32, found [n] u8.
 * Row i is the crate's fetch_embedding(ids[i]) bit for bit: the first occurrence of the id in (cluster, position) order,
 * decoded, reconstructed in rotated space and inverse-rotated.  A missing id gives a zero row and found[i] = 0.
 * Served from the first replica (it keeps the reconstruction factors).  The ids go through page-locked staging in chunks,
 * so device memory stays bounded for any n.  The first fetch of a handle builds its id map (12 bytes per vector, kept
 * until destroy).  Re-entrant; a fetch only reads the index, so searches may run alongside it.
 * Errors: RBQ_INVALID_CONFIG for a handle without reconstruction factors (rbq_index_create), a RBQ_ROTATOR_NONE handle,
 * or null pointers when n > 0; RBQ_DEVICE.  n == 0 returns RBQ_OK; on an empty index every id is not found. */
int rbq_index_fetch_embeddings(const rbq_index* idx, const uint64_t* ids, uint64_t n, float* out, uint8_t* found);
/* The same on device pointers, ENQUEUED on `hip_stream` (NULL = default stream) without host synchronisation (the first
 * call of a handle may block while the id map is built).  d_ids must be device memory of the first replica's device. */
int rbq_index_fetch_embeddings_device(const rbq_index* idx, const uint64_t* d_ids, uint64_t n, float* d_out,
                                      uint8_t* d_found, void* hip_stream);

/* Page-locked host memory for query / result buffers: rbq_search_batch DMA-s such buffers directly. */
void* rbq_host_alloc(size_t bytes);
void rbq_host_free(void* p);

/* OPTIONAL full-precision rerank — an extension (BASELINE north_star item 3), NOT reference behaviour: the
 * reference index stores no raw vectors (src/ivf.rs:207-242) and never re-scores.  Default OFF; results are
 * reference-identical only while it is off.  `vectors` [n][dim] f32 (HOST: copied to every replica; DEVICE pointer
 * on the replica's device: borrowed, must outlive the index) indexed by id; passing NULL detaches.  While enabled,
 * every search re-scores its returned ids with the exact l2_distance_sqr / dot (canonical order of
 * src/math.rs:154-245) against these vectors and re-sorts them; ids >= n get NaN.  top_k <= 1024.
 * Toggle with rbq_debug_set_option(idx, "rerank", 0/1) once vectors are attached (attaching switches it on).
 * Pool: rbq_debug_set_option(idx, "rerank_pool", v), on every replica, with or without vectors attached.  v <= 0 stores 0
 * (the default: everything above); v > 4096 is RBQ_INVALID_CONFIG.  While the rerank is on and v > top_k >= 1, every search
 * entry (rbq_search_batch on every replica, rbq_search_batch_device on the caller's stream) returns per query: the POOL is
 * what the same call returns with top_k := v and the rerank off (same nprobe, filter, numeric variant and options; `diag`
 * is that call's), entries (id, rank r) for r = 0 .. c-1, c <= v; each is scored exactly as above (ids >= n get the NaN
 * 0x7fc00000); the entries are ordered by f32::total_cmp of the exact score (descending for inner product: NaN then
 * comes first), then by r; the first min(top_k, c) are written, out_counts is their number, unused slots are UINT64_MAX /
 * NaN.  For v <= 1024 that is the first top_k entries of the unpooled rerank's result at top_k := v, bit for bit.  The
 * bounds on top_k (2^20, 8 GiB of heap workspace) are then evaluated for v, and top_k itself may exceed 1024.  With
 * v <= top_k nothing changes, the refusal of top_k > 1024 with the rerank on included. */
int rbq_index_set_rerank_vectors(rbq_index* idx, const float* vectors, uint64_t n);
/* Rows in 16 bits.  No entry point is added for them: the option "rerank_raw_dtype" (rbq_debug_set_option, every replica; the
 * default is RBQ_RAW_F32) says what the pointer of the NEXT rbq_index_set_rerank_vectors holds — rows of `dim` elements of that
 * type, dim * sizeof(element) bytes apart, passed through the `const float*` parameter as they are.  Any other value is
 * RBQ_INVALID_CONFIG (detail set) and the handle keeps what it had; rows already attached keep the type they were attached with.
 * rbq_debug_copy_index(idx, "rerank_raw_dtype", &v, 4) reads the RBQ_RAW_* of the attached rows as one int32, -1 with none.
 * A 16-bit element is widened to f32 EXACTLY where a kernel loads it (f16 subnormals, signed zeros, infinities and quiet
 * NaNs included; bf16 is bits << 16) and enters the same canonical sums, multiply and add unfused: a search over 16-bit rows X16
 * returns, bit for bit (ids, counts, score bits), what it returns with widen(X16) attached as f32, pooled or not, on every
 * search entry.  A signalling NaN scores some NaN.  The library never rounds: rounding f32 data to 16 bits is the caller's choice
 * and the caller's recall.  A borrowed device pointer to 16-bit rows must be 2-byte aligned (else RBQ_INVALID_CONFIG); rows that
 * all start 4-byte aligned (base 4-byte aligned and dim even) are read 16 bytes per lane, any others element by element, with the
 * same results, slower.  Nothing outside [vectors, vectors + n * dim * sizeof(element)) is read. */
/* element types of 16-bit rows (and f32, the default of both options): the values of "rerank_raw_dtype" and of "query_dtype" */
#define RBQ_RAW_F32  0
#define RBQ_RAW_F16  1   /* IEEE binary16 */
#define RBQ_RAW_BF16 2   /* upper 16 bits of an f32 */

/* Numeric variant: which build of the reference the kernels reproduce bit for bit.  The reference picks its arithmetic at
 * compile time (cfg(target_feature) in src/simd.rs), so two builds of it return different last bits of the scores:
 *   RBQ_NUMERIC_NATIVE_AVX512 (default)  the crate built in its own checkout (.cargo/config.toml: target-cpu=native) on an
 *                                        AVX-512 host
 *   RBQ_NUMERIC_NATIVE_AVX2              the same on an AVX2-only host (the AVX2 body of the ex-code dot product)
 *   RBQ_NUMERIC_PORTABLE                 RUSTFLAGS="" builds: a crates.io dependency, the PyPI wheel, on x86-64 hosts with AVX2
 *                                        (the scalar bodies of the ex-code dot product and of the estimator's first operation)
 * Out of scope: x86-64 hosts without AVX2 (math.rs then takes its SSE2 bodies), non-x86 hosts, and builds with
 * -C llvm-args=--ffast-math.  INTEGRATION.md, "Which arithmetic to pick".  The setting applies to every replica; like every other
 * option it is not synchronised with calls already in flight.  Any other value: RBQ_INVALID_CONFIG (detail set). */
#define RBQ_NUMERIC_NATIVE_AVX512 0
#define RBQ_NUMERIC_NATIVE_AVX2   1
#define RBQ_NUMERIC_PORTABLE      2
int rbq_index_set_numeric_variant(rbq_index* idx, int variant);
/* The handle's numeric variant (RBQ_NUMERIC_*), or -1 for a null handle. */
int rbq_index_numeric_variant(const rbq_index* idx);

/* Timing taps for bench.py: average duration (ms) of each stage kernel between
 * rbq_profile_begin/end, measured with hipEvents on the stream the kernels run
 * on. stage names: "prep", "rank", "select", "scan". Returns <0 for an unknown stage. */
void   rbq_profile_begin(rbq_index* idx);
void   rbq_profile_end(rbq_index* idx);
double rbq_profile_stage_ms(const rbq_index* idx, const char* stage, uint64_t* launches);
/* Durations (ms) of the individual timed launches of a stage, in launch order (replica after replica); returns their
 * number, writes at most `cap` of them to `out` (which may be NULL). */
uint64_t rbq_profile_stage_samples(const rbq_index* idx, const char* stage, float* out, uint64_t cap);
/* Algorithmic bytes (sum over probed lists of n_c*(D/8+12)) of the
 * scan launches between rbq_profile_begin/end. */
uint64_t rbq_profile_scan_bytes(const rbq_index* idx);
/* Traffic counters of the scan launches between rbq_profile_begin/end (summed over replicas), out[0..n):
 *   [0] vectors probed (sum of n_c over probed lists)   [1] block records whose sign codes were requested
 *   [2] block records whose factor rows were requested  [3] block-stream entries read (16 B each)
 *   [4] candidates whose ex codes were fetched          [5] queries scanned                */
int rbq_profile_counters(const rbq_index* idx, uint64_t* out, uint32_t n);
/* Which stages rbq_profile_begin/end time: bit 0 prep, 1 rank, 2 select, 3 scan (default: all four). Every timed
 * stage costs two event records per launch; a throughput measurement that only needs the dominant kernel's
 * duration selects that stage alone. */
void rbq_profile_select_stages(rbq_index* idx, uint32_t mask);
/* Time only every n-th launch of each selected stage (default 1 = every launch). */
void rbq_profile_set_sampling(rbq_index* idx, uint32_t every);
/* Number of queries (since creation) whose probe selection fell back from the MFMA shortlist to the
 * all-lists canonical ranking (shortlist overflow / non-finite scores). Diagnostic. */
uint64_t rbq_debug_rank_fallbacks(const rbq_index* idx);
/* tie log of k_scan (queries whose result depends on the layout of the reference's BinaryHeap, src/ivf.rs:904-931, replay their logged
   candidates instead of their lists): out4 = replays, log entries replayed, real heap operations among them, logs that overflowed */
void rbq_debug_tie_log_stats(const rbq_index* idx, uint64_t* out4);
/* Diagnostic: which kernel instantiation each stage (prep, rank, select, scan) launches for a call of nq queries with this top_k /
 * nprobe on this index, and what it occupies: out[stage][6] = workgroups, threads per workgroup, VGPRs per lane, LDS bytes per
 * workgroup (static + dynamic), scratch bytes per lane, 0.  Nothing is launched.  bench.py's `regime` object is built from it. */
int rbq_debug_stage_resources(rbq_index* idx, uint64_t nq, uint32_t top_k, uint32_t nprobe, uint32_t* out);
/* Replica arrays (process-wide, since start) that were copied between devices through the page-locked bounce buffer instead of
 * hipMemcpyPeer: the path taken when the runtime refuses the peer copy, or for every replica copy when RBQ_FORCE_NO_PEER=1 is in
 * the environment (test switch: the only way the path can run on a one-GPU box). Diagnostic. */
uint64_t rbq_debug_bounce_copies(void);
/* Exact head evaluation of the lazy probe selection (since creation): queries for which it ran / times its geometry guard tripped
 * (must stay 0). Diagnostic. */
uint64_t rbq_debug_head_exact_evaluations(const rbq_index* idx);
uint64_t rbq_debug_head_exact_guard_trips(const rbq_index* idx);
/* Number of queries (since creation) that met two bit-identical distances in their top-k and were therefore
 * re-run inside the scan kernel with the exact BinaryHeap emulation (src/ivf.rs:2078-2105 pushes into a
 * std BinaryHeap, whose tie behaviour depends on its layout). Diagnostic. */
uint64_t rbq_debug_heap_restarts(const rbq_index* idx);
/* Diagnostic: copy one of the index's device arrays ("blocks", "ids", "ex", "fadd_ex", "fres_ex", "bsum", "lsum", "bsumx",
 * "centroids", "list_gb0", "list_n"; the ranking GEMM's operand "cent_hl" — the split-bf16 image of the centroids as the device
 * keeps it, [nlist][2 D] u16 with the 32 hi and the 32 lo values of every 32-element K slab side by side (one 128-byte line per row
 * and slab) — and its logical planes "cent_hi", "cent_lo", [nlist][D] u16, de-interleaved by the copy; "cnorm2", [nlist] f32) to the
 * host; `bytes` must be the array's exact size. */
int rbq_debug_copy_index(rbq_index* idx, const char* name, void* dst, uint64_t bytes);
/* test hook: t of best_rescale_factor for n rows of o = |r_i| / norm(r) (host [n][dim] f32, every value in [0, 1];
 * dim <= 2048, 1 <= ex_bits <= 7) -> out_t [n] f64, computed by the device encoder's kernel */
int rbq_debug_best_rescale(const float* o_abs, uint64_t n, uint32_t dim, uint32_t ex_bits, int device, double* out_t);
/* Diagnostic: copy an intermediate buffer ("rot", "lut", "consts", "scores", "probe", "nstream", "wl", "nvec", "dead_skipped",
 * "audit_dead", "head_ub"; "rot_hl": the split-bf16 image of the rotated queries, [nq][2 D] u16 in the layout of "cent_hl", written only
 * when the split-bf16 ranking GEMM serves the call, and "rot_hi", "rot_lo": its planes, [nq][D] u16, de-interleaved by the copy) of the
 * workspace that rbq_search_batch_device bound to `hip_stream`; the caller has synchronised
 * that stream. */
int rbq_debug_copy_workspace(rbq_index* idx, void* hip_stream, const char* name, void* dst, uint64_t bytes);
/* Diagnostic switches; results are identical under every setting, only the work done changes:
 *   "block_bound" 0      stream every probed block (no block-level lower-bound skipping)
 *   "exact_rank" 1       rank all nq x nlist pairs in canonical order instead of the MFMA shortlist
 *   "force_rank_fallback" 1   send every query through the shortlist's all-lists fallback
 *   "f32_rank" 1         approximate list scores from the f32 MFMA GEMM instead of the split-bf16 one
 *   "wg_prep" 1          workgroup-per-query query preparation for every rotator (default: one wave per query)
 *   "exact_heap" 1       keep the top-k in the BinaryHeap emulation from the first candidate (no sorted fast path)
 *   "lazy_select" 0      score and stream every probed list (default 1: lists that are provably skipped as a whole —
 *                        every lower bound of the list at or above a select-time upper bound of the k-th distance — are
 *                        neither scored exactly nor streamed; their sizes still count in skipped_by_lower_bound)
 *   "profile_counters" 0 an open profile (rbq_profile_begin) keeps its stage timings but not the traffic counters (default 1; the
 *                        counters cost a pipelined caller 2-3 %: bench.py times without them and counts in a pass of its own)
 *   "latency_path" 0     small calls through the batch kernels (default 1: calls of up to 4 queries rotate the query, build its LUT and
 *                        score every list exactly in ONE launch; batches up to 512 queries are prepared by a workgroup per query)
 *   "tie_log" 0          a query with equal distances in its top-k is scanned again with the BinaryHeap emulation (default 1: k_scan
 *                        logs the candidates it refines — 12 B each, up to 8192 per query in the calling stream's workspace — and the
 *                        tied query replays the log; rbq_debug_tie_log_stats)
 *   "scan_wave" 0/1/2    which scan kernel serves a call
 *   "ub_tap" 1           the lazy selection exports its head bounds to the workspace buffer "head_ub", [nq][778] u32 per call (default
 *                        0: nothing is written): ncand, the number of head lists h, the g_add / g_err bits each head list's bounds
 *                        used (4 pairs), then per head candidate block (gblock, bits of its bound U, real vectors); ncand = 0 where
 *                        the lazy path was not entered.  T_ub is the smallest finite U whose blocks of U' <= U hold top_k vectors
 *   "rank_ksplit" 0      never split the K loop of the ranking GEMM (default 1: calls of up to 256 queries split it 2-4 ways over
 *                        grid.z, the parts added atomically to a cleared row; n > 1 forces min(n, 4) parts, the most the
 *                        shortlist's error bound is derived for)
 *   "rank_planar" 1      TEST ONLY: the split-bf16 ranking GEMM reads planar copies of its operands (two planes [rows][D] each,
 *                        de-interleaved per call) instead of the interleaved images — same kernel, same scores bit for bit
 * and ten that are not result-neutral:
 *   "query_dtype" v      RBQ_RAW_F32 (0, default), RBQ_RAW_F16 or RBQ_RAW_BF16, on every replica: what every entry point that takes
 *                        queries on this handle — rbq_search_batch (one replica or several), rbq_search_batch_device,
 *                        rbq_posting_scan_batch, rbq_mstg_search_batch / _device, rbq_mstg_search_refined_batch / _device — reads
 *                        its `queries` / `d_queries` pointer as: nq rows of query_dim elements of that type (2 * query_dim bytes
 *                        apart for the 16-bit types), see rbq_search_batch.  Any other value is RBQ_INVALID_CONFIG (detail set)
 *                        and the handle keeps what it had.  rbq_debug_copy_index(idx, "query_dtype", &v, 4) reads it back as one
 *                        int32.  It composes with the filter, diag, range search, the rerank (pooled or not, raw rows of any
 *                        type), every numeric variant and every diagnostic option; a call in flight while it changes is the
 *                        caller's problem.  Contract: ids, counts, score bits, diag, list outputs and errors of a call with 16-bit
 *                        queries equal those of the same call with "query_dtype" RBQ_RAW_F32 on the rows widened to f32
 *   "rerank" 0/1         the optional full-precision rerank (needs rbq_index_set_rerank_vectors)
 *   "rerank_pool" v      candidates the rerank re-scores per query, 0 = off, at most 4096 (rbq_index_set_rerank_vectors)
 *   "mstg_rerank" 0/1    exact rerank of the MSTG candidate pool (default 0; rbq_mstg.h, rbq_mstg_search_refined_batch): the refined
 *                        MSTG entries, and only they, reduce the pool to one entry per id and score it exactly against the
 *                        attached raw rows.  Needs raw vectors attached and "rerank" 1, else the refined call is
 *                        RBQ_INVALID_CONFIG; may be set with or without vectors attached.  rbq_debug_copy_index(idx, "mstg_rerank",
 *                        &v, 4) reads it back as one int32
 *   "range_radius_bits" v  the 32 bits of an f32 radius r, passed through the int (every pattern is accepted; default +inf)
 *   "range_search" 0/1   range search (default 0): rbq_search_batch / rbq_search_batch_device return every vector of the probed
 *                        lists with distance < r (L2) or score > r (inner product), see rbq_search_batch; RBQ_INVALID_CONFIG
 *                        while the rerank is on and "range_exact" is 0; the MSTG entry points and MSTG handles ignore it
 *   "range_exact" 0/1    exact range search (default 0; see rbq_search_batch): while "range_search" is 1, the estimate's matches
 *                        at r are candidates, scored exactly against the attached raw rows and kept iff exact distance < x (L2)
 *                        or exact dot product > x (inner product).  Needs raw vectors attached and "rerank" 1, else the search is
 *                        RBQ_INVALID_CONFIG; no effect while "range_search" is 0; MSTG handles ignore it
 *   "range_exact_radius_bits" v  the 32 bits of the f32 x, passed through the int (every pattern is accepted; default +inf)
 *   "numeric_variant" v  rbq_index_set_numeric_variant(idx, v): which build of the reference the scores reproduce
 *   "debug_replica" r    which replica rbq_debug_copy_index / rbq_debug_copy_workspace read */
int rbq_debug_set_option(rbq_index* idx, const char* name, int value);

/* Process-wide defaults: kept for ABI compatibility.  It used to raise the HIP hardware-queue count in the process environment; the
 * queue count is the host's choice (the HIP runtime's default, or GPU_MAX_HW_QUEUES set by the host before the first HIP call), and
 * this call now leaves the environment untouched.  Returns RBQ_OK. */
int rbq_process_defaults(void);
const char* rbq_strerror(int code);
/* Copies the calling thread's last error detail (e.g. "checksum mismatch",
 * "expected 960, got 128") into buf; returns its full length. */
int rbq_last_error_detail(char* buf, size_t n);

/* Library/ABI version (major<<16 | minor). */
uint32_t rbq_abi_version(void);

#ifdef __cplusplus
}
#endif

/* The brute-force index (BruteForceRabitqIndex): rbq_bf_* in the companion header. */
#include "rbq_bf.h"
/* The device k-means (run_kmeans_with_config): rbq_kmeans_device in its own header. */
#include "rbq_kmeans.h"
#include "rbq_persist.h"
/* Growing a device-resident index (FAISS-style add): rbq_index_append in its own header. */
#include "rbq_append.h"
/* Shrinking a device-resident index (FAISS-style remove_ids): rbq_index_remove_ids in its own header. */
#include "rbq_remove.h"

#endif /* RBQ_H */
