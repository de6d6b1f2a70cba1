/*
 * rbq_remove.h — C ABI of shrinking a device-resident IVF index: FAISS-style `remove_ids` on the GPU.  Included by rbq.h; kept in
 * a header of its own, like rbq_append.h.
 *
 * Before it a vector could only be dropped by rebuilding the index over the rows that stay (rbq_index_build_device_ex), which
 * needs every raw row resident again and is not possible at all for an index loaded from an RBQ1 stream.  rbq_index_remove_ids
 * takes a handle — built by any path, appended to, or loaded — and returns a NEW handle that holds every vector whose id is not
 * in a set.  Nothing is encoded again: every surviving vector keeps its bits, and the call is a stream compaction of the index
 * arrays inside each list.  The contract: with K the rows of X whose id is not in the set, ascending,
 * the result equals, array for array and byte for byte, the index rbq_index_build_device_ex builds over X[K] with a[K], the same
 * centroids, header and rescale mode — except that `ids` holds the original id of row K[j] where that build holds j.  Survivors
 * keep their order within a list, lists stay in order, block j of a list is its j-th run of 32 survivors, and the pad lanes of
 * every tail block hold the builder's fill (zeros, ids of all ones), never bytes of the source.  (The pad lanes of a LOADED
 * handle may hold the file's bytes: they are not carried either; for such a handle the contract is on the saved bytes and on
 * search results.)
 *
 * Device memory at the peak: the old index, the new index, 8 bytes per id of the set (twice: the caller's or the uploaded copy
 * and the sorted one, plus the sort's scratch), and the tables: 4 bytes per new slot (the slot map), 16 bytes per old block
 * (list, vector count, keep mask, scan) and 8 bytes per new block (list, vector count).
 */
#ifndef RBQ_REMOVE_H
#define RBQ_REMOVE_H

#include <stddef.h>
#include <stdint.h>

#include "rbq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Remove from `idx` every vector whose id is in `ids`.  `idx` is only read and stays valid (it may serve searches and fetches
 * during the call); the caller destroys both handles.  The new handle is built on the device of idx's first replica and
 * replicated over `devices` as by rbq_index_append (devices[0] must be that device; NULL / n_devices <= 1 = that device only).
 *   ids          [n_ids] u64, HOST or DEVICE memory (detected).  Their order does not matter and repeats are allowed; an id that
 *                is not stored is ignored.  EVERY slot whose id is in the set goes: an index loaded from a stream may hold an id
 *                more than once.
 *   out_removed  NULL, or receives the number of slots removed
 * If nothing matches, the result equals idx.  A list may become empty.  If the set covers EVERY vector the call is refused with
 * a detail: rbq_index_build_device_ex refuses zero rows ("no vectors") and no other path makes a handle without vectors either.
 * Centroids, rotator and header are those of idx bit for bit.  The new handle takes over idx's numeric variant; debug options
 * start at their defaults; rerank vectors are not carried.  rbq_index_id_bound of the new handle is found on first use by the
 * reduction over its ids (1 + the largest id that stayed); it is not inherited.
 * Errors (*out = NULL, idx untouched): RBQ_INVALID_CONFIG with a detail for, checked in this order before the first HIP call,
 * a null idx / out, a posting-list handle (RBQ_ROTATOR_NONE), a handle without reconstruction factors (rbq_index_create), null
 * ids, n_ids == 0, a bad device list; and, found on the device before the new arrays are allocated, a set that covers every
 * vector.  Device failures are RBQ_DEVICE. */
int rbq_index_remove_ids(const rbq_index* idx, const uint64_t* ids, uint64_t n_ids,
                         int n_devices, const int* devices, uint64_t* out_removed, rbq_index** out);

/* MEASUREMENT ONLY, process-wide: device time in nanoseconds of the gather kernel of the last rbq_index_remove_ids
 * (tools/remove_rate.py divides the bytes it moved by it); 0 before the first one. */
uint64_t rbq_debug_remove_gather_ns(void);

#ifdef __cplusplus
}
#endif

#endif /* RBQ_REMOVE_H */
