/*
 * rbq_bf_mutate.h — C ABI of growing, shrinking and reading back a device-resident brute-force index: `add`, FAISS-style
 * `remove_ids` and `fetch_embedding` for rbq_bf_index.  Included by rbq_bf.h; kept in a header of its own, like rbq_append.h and
 * rbq_remove.h for the IVF index.
 *
 * Before it the brute-force index was frozen at training time: to add one vector a caller kept every raw row and trained again,
 * and a handle loaded from an RBF1 stream, which holds no raw rows, could not be changed or read back at all.
 * BruteForceRabitqIndex::train quantises every vector on its own against the zero centroid (src/brute_force.rs:252-273), so a
 * grown or shrunk index has an exact definition: it is the index `train` gives over the rows it then holds (DESIGN.md section
 * 25).  Both calls return a NEW handle; the input handle is only read, stays valid and may serve searches during the call; the
 * caller destroys both.  Everything runs on the handle's one device.
 *
 * Device memory at the peak: the old index and the new index, plus for an append the encoder's scratch of one chunk, and for a
 * removal 4 bytes per surviving row (the row map).  Before the new arrays of a removal are allocated it holds 9 bytes per old
 * row (keep mask, ranks, the scan's scratch) and 8 bytes per id of a host caller's set, freed again before the gather.
 */
#ifndef RBQ_BF_MUTATE_H
#define RBQ_BF_MUTATE_H

#include <stddef.h>
#include <stdint.h>

#include "rbq_bf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Append `count` rows to `idx`: row i gets id rbq_bf_len(idx) + i.
 * Contract: with X_old the rows the handle was trained on, the result equals, array for array and bit for bit,
 * rbq_bf_train_device(hdr, X_old ++ X_new, rescale, t_const), so rbq_bf_save_rbf1 writes the same stream for both.  Nothing old is
 * encoded again: the old arrays are carried by device-to-device copies into arrays of len + count rows, and the encoder chain of
 * rbq_bf_train_device fills rows len .. at their offsets.
 *   vectors  [count][dim] f32 in host or device memory (detected, as rbq_bf_train_device does; host rows are copied a chunk at a
 *            time).  Finite values only: there is no finite check, as for the encoders.
 *   rescale, t_const  as for rbq_bf_train_device.  A handle does not remember what it was encoded with and RBF1 does not store
 *            it: the caller passes the mode (and constant) of the old rows to get the index `train` gives over all rows.
 *   max_chunk_rows    as for rbq_bf_train_device; the result does not depend on it.
 * The new handle's ex_len (rbq_bf_view::ex_len) is idx's: a trained 1-bit handle carries padded_dim/8 zero bytes of ex code per
 * vector and a created one may carry none; the contract is on the saved bytes.
 * Errors (*out = NULL, idx untouched): RBQ_INVALID_CONFIG with a detail for, checked in this order before the first HIP call, a
 * null idx / out, null vectors, count == 0, len + count above the 2^32 - 1 vectors a handle holds ("more than 2^32 vectors"), an
 * unknown rescale mode, RBQ_RESCALE_CONST with ex_bits > 0 and t_const not > 0.  Device failures are RBQ_DEVICE. */
int rbq_bf_append(const rbq_bf_index* idx, const float* vectors, uint64_t count, int rescale, float t_const,
                  uint64_t max_chunk_rows, rbq_bf_index** out);

/* Remove from `idx` every vector whose id is in `ids`.  The brute-force index has no id array and RBF1 stores none: the id of a
 * vector IS its position.  So this is FAISS IndexFlat::remove_ids: survivors keep their order and are RENUMBERED 0 .. len' - 1 — the
 * id of every vector behind a removed one changes.
 * Contract: with K the positions not in the set, ascending, the result equals rbq_bf_train_device over X[K], bit for bit, saved
 * bytes included.  Nothing is encoded again: the call is a stream compaction of the flat arrays (a mark kernel scatters the set
 * into a keep mask, a scan ranks the survivors, one gather kernel moves the sign codes, the ex codes and the eight factor arrays).
 *   ids          [n_ids] u64, HOST or DEVICE memory (detected).  Any order, repeats allowed; an id >= len is ignored.
 *   out_removed  NULL, or receives the number of rows removed
 * If nothing matches, the result equals idx.  A set that covers EVERY vector is refused with a detail, as rbq_index_remove_ids
 * does: `train` refuses zero rows.
 * Errors (*out = NULL, idx untouched): RBQ_INVALID_CONFIG with a detail for, in this order before the first HIP call, a null
 * idx / out, null ids, n_ids == 0; and, found on the device before the new arrays are allocated, a set that covers every vector.
 * Device failures are RBQ_DEVICE. */
int rbq_bf_remove_ids(const rbq_bf_index* idx, const uint64_t* ids, uint64_t n_ids, uint64_t* out_removed,
                      rbq_bf_index** out);

/* The brute-force counterpart of rbq_index_fetch_embeddings: row i of `out` is the crate's IVF fetch_embedding
 * (src/ivf.rs:1247-1307) of vector ids[i] evaluated against the brute-force index's zero centroid, bit for bit:
 * code[j] = ex[j] + (bit[j] << ex_bits); rotated[j] = (0.0f + delta * (float)code[j]) + vl; then inverse_rotate_into of either
 * rotator.  out [n][dim] f32, found [n] u8; an id >= len gives a zero row and found = 0; repeats are served.  Host buffers; the
 * call works in chunks within a fixed scratch budget (64 MiB) and returns when `out` is complete.  n == 0 returns RBQ_OK. */
int rbq_bf_fetch_embeddings(const rbq_bf_index* idx, const uint64_t* ids, uint64_t n, float* out, uint8_t* found);
/* The same from device buffers of the handle's device, enqueued on `hip_stream` (a hipStream_t; NULL = the default stream)
 * without host synchronisation: the results are complete when the stream reaches the end of the enqueued work. */
int rbq_bf_fetch_embeddings_device(const rbq_bf_index* idx, const uint64_t* d_ids, uint64_t n, float* d_out,
                                   uint8_t* d_found, void* hip_stream);

/* MEASUREMENT ONLY, process-wide: device time in nanoseconds of the carry copies (old arrays into the grown ones) of the last
 * rbq_bf_append, and of the gather kernel of the last rbq_bf_remove_ids (tools/bf_mutate_rate.py divides the bytes they moved by
 * it); 0 before the first one. */
uint64_t rbq_bf_debug_append_carry_ns(void);
uint64_t rbq_bf_debug_remove_gather_ns(void);

#ifdef __cplusplus
}
#endif

#endif /* RBQ_BF_MUTATE_H */
