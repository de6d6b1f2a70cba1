/*
 * rbq_mstg_mutate.h — C ABI of changing a device-resident MSTG index: `add` and `remove_ids` on posting-list handles
 * (rotator RBQ_ROTATOR_NONE).  Included by rbq_mstg.h; the IVF counterparts are rbq_append.h and rbq_remove.h, which keep
 * refusing posting-list handles.
 *
 * Before it an MSTG index was immutable: new rows meant rbq_mstg_build_device over every raw row again, and an index loaded
 * from a `.mstg` file, which has no raw rows, could not change at all.  Both calls take a handle — built, loaded, or the result
 * of an earlier call — and return a NEW handle.  The contract: ClosureAssigner::assign depends only on
 * the row and the centroids, so appending X_new to the index over X_old equals, array for array and byte for byte,
 * rbq_mstg_build_device over X_old ++ X_new with the same centroids, and removing a set equals that build over the rows that
 * stay, with their original ids.  Lists only grow or shrink: nothing is re-clustered, and a list that outgrows the
 * max_posting_size it was clustered for is not split.
 */
#ifndef RBQ_MSTG_MUTATE_H
#define RBQ_MSTG_MUTATE_H

#include <stddef.h>
#include <stdint.h>

#include "rbq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Append `count` rows to the posting lists of `idx`.  `idx` is only read and stays valid (it may serve searches during the
 * call); the caller destroys both handles.  Everything runs on the device of idx's first replica.
 *   vectors    [count][dim] f32, HOST or DEVICE memory (detected; host rows are copied a chunk at a time).  Row i gets the id
 *              first_id + i; first_id >= rbq_index_id_bound(idx).
 *   closure_epsilon, max_replicas   the lists of row i are ClosureAssigner{closure_epsilon, max_replicas}.assign(row,
 *              centroids) with the handle's centroids, read in device memory; arithmetic, sort and RNG rule are those of
 *              rbq_mstg_closure_assign, bit for bit.  A row becomes one slot in each of its lists; the slots share its id.
 *   max_chunk_rows   upper bound on the rows per closure pass and per encode pass; 0 = as many as the 512 MiB workspaces
 *              hold (the encode pass is sized by (row, list) pairs).  The result does not depend on it.
 *   out_lists  NULL, or [count][max_replicas] u32; out_counts NULL, or [count] u32: given together, both host or both device
 *              memory; conventions as rbq_mstg_closure_assign (closest list first, unused slots UINT32_MAX).
 * The rescale mode is not an argument: the new rows are encoded with what the handle's lists were built with — the constant
 * t_const it remembers (RBQ_RESCALE_CONST), else the per-vector factor (RBQ_RESCALE_OPTIMAL); moot for a 1-bit index.  The new
 * handle holds idx's centroids bit for bit, its t_const and numeric variant, the residual norms of old and new slots, and
 * records the id bound first_id + count.  Every list stays in ascending id order.
 * Errors (*out = NULL, idx untouched): RBQ_INVALID_CONFIG with a detail for, in this order before the first HIP call, a null
 * idx / out, a handle that is not a posting-list handle, a posting-list handle without residual norms or reconstruction
 * factors (rbq_index_create*), null vectors, count == 0, max_replicas == 0 or > RBQ_MSTG_MAX_REPLICAS, an epsilon that is
 * negative or not finite, out_lists and out_counts in different memories; and, found on the device before the new arrays are
 * allocated, first_id below the id bound, first_id + count passing 2^64 - 1, a non-finite value in `vectors`, more than
 * 2^32 - 16 slots in total.  Device failures are RBQ_DEVICE. */
int rbq_mstg_append(const rbq_index* idx, const float* vectors, uint64_t count, uint64_t first_id,
                    float closure_epsilon, uint32_t max_replicas, uint64_t max_chunk_rows,
                    uint32_t* out_lists, uint32_t* out_counts, rbq_index** out);

/* Remove from the posting lists of `idx` every slot whose id is in `ids`, in every list that holds it.  Arguments and set
 * semantics are those of rbq_index_remove_ids (ids [n_ids] u64 in host or device memory, any order, repeats allowed, ids that
 * are not stored ignored), on the device of idx's first replica.  Nothing is encoded again.
 *   out_removed  NULL, or receives the number of SLOTS removed: a vector held by three lists counts three
 * A list may become empty; a set that covers every vector is refused.  The new handle holds idx's centroids bit for bit, the
 * residual norms of the slots that stay, its t_const and numeric variant.
 * Errors (*out = NULL, idx untouched): RBQ_INVALID_CONFIG with a detail for, in this order before the first HIP call, a null
 * idx / out, a handle that is not a posting-list handle, a posting-list handle without residual norms or reconstruction
 * factors, null ids, n_ids == 0; and, found on the device, a set that covers every vector.  Device failures are RBQ_DEVICE. */
int rbq_mstg_remove_ids(const rbq_index* idx, const uint64_t* ids, uint64_t n_ids, uint64_t* out_removed, rbq_index** out);

/* TEST ONLY, process-wide: encode passes of every rbq_mstg_append so far. */
uint64_t rbq_debug_mstg_append_passes(void);

#ifdef __cplusplus
}
#endif

#endif /* RBQ_MSTG_MUTATE_H */
