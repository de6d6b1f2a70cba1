/*
 * rbq_bf.h — C ABI of the brute-force index, the MI355X counterpart of lqhl/rabitq-rs's
 * `BruteForceRabitqIndex` (reference src/brute_force.rs).  Included by rbq.h; kept in a header of its own so
 * that rbq.h stays the IVF path's boundary (integration/gpu_ivf.rs binds exactly that one).
 */
#ifndef RBQ_BF_H
#define RBQ_BF_H

#include <stddef.h>
#include <stdint.h>

#include "rbq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- brute-force index: BruteForceRabitqIndex (reference src/brute_force.rs) ------------------------------------------
 * Every vector is evaluated for every query: no clustering, no FastScan LUT, two sequential f32 dot products per vector
 * (search_internal, src/brute_force.rs:545-650).  The index lives on one device.  Its header is an rbq_header with
 * n_lists ignored (rotator MATRIX or FHT_KAC; ex_bits 0, 2 or 6; padded_dim % 16 == 0 and <= 2048). */
typedef struct rbq_bf_index rbq_bf_index; /* opaque; owns device memory on one GPU */

/* The index's per-vector arrays (QuantizedVector, src/quantizer.rs), borrowed for the duration of the call; ids are 0..n-1. */
typedef struct {
    uint64_t       n;
    const uint8_t* bin_codes;     /* [n][padded_dim/8] binary_code_packed (MSB-first)                          */
    const uint8_t* ex_codes;      /* [n][ex_len] ex_code_packed; may be NULL when ex_len == 0                 */
    uint64_t       ex_len;        /* bytes of ex code per vector: padded_dim*ex_bits/8, or for ex_bits == 0 either
                                     0 or padded_dim/8 (the zero bytes of a freshly trained 1-bit index, which
                                     save_to_writer writes: rbq_bf_save_rbf1 reproduces them)                   */
    const float*   delta;         /* [n] each                                                                  */
    const float*   vl;
    const float*   f_add;
    const float*   f_rescale;
    const float*   f_error;
    const float*   residual_norm;
    const float*   f_add_ex;
    const float*   f_rescale_ex;
} rbq_bf_view;

/* Upload an index (device = HIP ordinal, -1 = the current device).  Inputs are copied; nothing is retained. */
int rbq_bf_create(const rbq_header* hdr, const rbq_bf_view* view, int device, rbq_bf_index** out);
/* BruteForceRabitqIndex::train (reference src/brute_force.rs:214-285) on the device: every row of `data` is rotated,
 * quantised against the zero centroid (quantize_with_centroid) in id order — the id of row i is i — and written straight
 * into the index's arrays in HBM.  The handle equals, array for array and bit for bit, rbq_bf_create over the CPU builder's
 * result for the same input, the padded_dim/8 zero bytes of ex code per vector of a 1-bit index (rbq_bf_view::ex_len)
 * included, so rbq_bf_save_rbf1 writes the same stream for both.
 *   hdr      dim, padded_dim, metric, rotator with its blob, ex_bits (0, 2 or 6); n_lists and n_vectors are ignored.  It
 *            gets the checks of rbq_bf_create.
 *   data     [n][dim] f32 in host or device memory (detected; host rows are copied a chunk at a time).  Finite values
 *            only: like the IVF device encoder, the result for NaN or infinite input is not specified.
 *   rescale  RBQ_RESCALE_CONST (RabitqConfig::faster: t_const > 0 required when ex_bits > 0) or RBQ_RESCALE_OPTIMAL
 *            (RabitqConfig::new: best_rescale_factor per vector, t_const ignored; moot at ex_bits == 0), as for
 *            rbq_index_build_device_ex.  Any other value is RBQ_INVALID_CONFIG.
 *   max_chunk_rows  upper bound on the rows rotated and encoded per pass (callers short of HBM); 0 = as many as the
 *            encoder's 512 MiB of rotated rows hold.  The result does not depend on it.
 * Errors: n == 0 is RBQ_INVALID_CONFIG "training data must be non-empty"; a null pointer is RBQ_INVALID_CONFIG; every
 * argument is checked before the first HIP call.  Never aborts: device failures are RBQ_DEVICE. */
int rbq_bf_train_device(const rbq_header* hdr, const float* data, uint64_t n, int rescale, float t_const,
                        uint64_t max_chunk_rows, int device, rbq_bf_index** out);
/* Build the index from an RBF1 byte stream (save_to_writer, src/brute_force.rs:305-386) with the validation of
 * load_from_reader (:395-520) incl. CRC-32.  Like the crate, it refuses the 1-bit streams the crate writes ("checksum
 * mismatch"): its writer stores padded_dim/8 bytes of ex code per vector that its reader does not read. */
int rbq_bf_load_rbf1(const void* bytes, size_t len, int device, rbq_bf_index** out);
/* save_to_writer, byte for byte, into a malloc'd buffer; free it with rbq_bf_free_bytes. */
int rbq_bf_save_rbf1(const rbq_bf_index* idx, uint8_t** bytes, uint64_t* len);
void rbq_bf_free_bytes(uint8_t* p);
void rbq_bf_destroy(rbq_bf_index* idx);
uint64_t rbq_bf_len(const rbq_bf_index* idx);
uint32_t rbq_bf_dim(const rbq_bf_index* idx);
uint32_t rbq_bf_padded_dim(const rbq_bf_index* idx);

/* search / search_filtered of BruteForceRabitqIndex for nq queries (the crate runs them one at a time).  Conventions of
 * rbq_search_batch: queries [nq][query_dim] host f32; out_ids / out_scores [nq][top_k] (unused slots UINT64_MAX / NaN);
 * out_counts [nq]; filter_words != NULL is search_filtered with a dense bitset of filter_nbits bits (bit i set <=>
 * filter.contains(i)).  L2: distance ascending; inner product: score = -distance, descending.  Ids, counts and score
 * bits equal the crate's, ties included.
 * Errors in the crate's order: EMPTY_INDEX, then DIMENSION_MISMATCH, then top_k == 0 returns RBQ_OK with all counts 0.
 * Supported: 1 <= top_k <= 16384 (top_k > 16384 is RBQ_INVALID_CONFIG); nq < 2^31.  Re-entrant on one handle (each call
 * has its own stream and workspace, at most 256 MiB: the batch is cut into sub-batches of queries and chunks of
 * vectors).  Never aborts: device failures are RBQ_DEVICE. */
int rbq_bf_search_batch(const rbq_bf_index* idx, const float* queries, uint64_t nq, uint32_t query_dim, uint32_t top_k,
                        const uint32_t* filter_words, uint64_t filter_nbits,
                        uint64_t* out_ids, float* out_scores, uint32_t* out_counts);
/* Diagnostic, since creation, summed over the queries of every call on this handle: out2[0] = candidates pushed into the
 * BinaryHeap emulation, out2[1] = those among them whose outcome depends on the heap's layout (a key equal to the root, or a
 * push made while equal keys sat on the heap's root-to-last-slot path: the ties of the reference's BinaryHeap). */
void rbq_bf_debug_heap_stats(const rbq_bf_index* idx, uint64_t* out2);
/* TEST ONLY, process-wide: at most `vectors` vectors per chunk of rbq_bf_search_batch; returns the previous value (0: the
 * default, as many as the 128 MiB distance workspace holds for one query, which 0 also restores).  A call reads it once,
 * before its first launch.  The budgets that size the query sub-batch are untouched and results do not depend on it: it
 * exists so that a test can run the several-chunk path (heap state carried between chunks) on a small index. */
uint64_t rbq_bf_debug_set_chunk_vectors(uint64_t vectors);
/* TEST ONLY, process-wide: selection launches of every rbq_bf_search_batch so far, one per (query sub-batch, vector chunk). */
uint64_t rbq_bf_debug_select_launches(void);

#ifdef __cplusplus
}
#endif

/* Growing, shrinking and reading back a brute-force index (rbq_bf_append, rbq_bf_remove_ids, rbq_bf_fetch_embeddings*). */
#include "rbq_bf_mutate.h"

#endif /* RBQ_BF_H */
