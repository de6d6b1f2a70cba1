/*
 * rbq_append.h — C ABI of growing a device-resident IVF index: FAISS-style `add` on the GPU.  Included by rbq.h; kept in a header
 * of its own, like rbq_kmeans.h.
 *
 * rbq_index_build_device_ex needs every vector at once and rbq_build_stream_begin* the final size of every list; neither takes
 * an existing handle.  rbq_index_append takes one — built by any path, or loaded from an RBQ1 stream, which holds no raw
 * vectors — and returns a NEW handle that holds its vectors and `count` more.  The contract: appending
 * rows X_new with lists a_new and ids n_old .. to the index over X_old / a_old gives, array for array and byte for byte, the
 * index rbq_index_build_device_ex builds over X_old ++ X_new with a_old ++ a_new, the same centroids, header and rescale
 * mode; rbq_index_save_rbq1 writes the same bytes for both.  (The padding lanes of a LOADED handle may hold the file's bytes:
 * for it the contract is on the saved bytes and on search results.)
 *
 * Device memory at the peak: the old index, the new index and at most about 1.2 GB of scratch.  The index does not grow in
 * place: that would have to exclude concurrent searches and every per-handle cache.
 */
#ifndef RBQ_APPEND_H
#define RBQ_APPEND_H

#include <stddef.h>
#include <stdint.h>

#include "rbq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Append `count` vectors to `idx`.  `idx` is only read and stays valid (it may serve searches and fetches during the call); the
 * caller destroys both handles.  The new handle is built on the device of idx's first replica and replicated over `devices` as
 * by rbq_build_stream_finish (devices[0] must be that device; NULL / n_devices <= 1 = that device only).
 *   vectors        [count][dim] f32, HOST or DEVICE memory (detected); host rows are copied a chunk at a time
 *   assign         [count] u32 list of every row, HOST or DEVICE (detected); NULL = the nearest centroid: the row is rotated by
 *                  the index's rotator and goes to the list minimising the canonical distance of DESIGN.md section 11 to the
 *                  rotated centroids (sequential unfused f32 norms and dot products in coordinate order,
 *                  (|x|^2 + |c|^2) - 2 dot clamped at 0, strict < in ascending list order: ties go to the lowest list)
 *   first_id       the id of row i is first_id + i; first_id >= rbq_index_id_bound(idx), so ids stay unique and every list
 *                  stays in ascending id order
 *   rescale, t_const   as for rbq_index_build_device_ex (a handle does not remember what it was built with; an RBQ1 stream
 *                  does not store it either)
 *   max_chunk_rows upper bound on the rows rotated, assigned and encoded per pass, rounded up to a multiple of 64;
 *                  0 = what the 512 MiB budgets give.  The result does not depend on it.
 *   out_assign     NULL, or [count] u32 in HOST or DEVICE memory (detected): the list every row went to
 * Centroids, rotator and header are those of idx bit for bit (the rotated centroids are copied, nothing is rotated again).  The
 * new handle takes over idx's numeric variant; debug options start at their defaults; rerank vectors are not carried.
 * Errors (*out = NULL, idx untouched): RBQ_INVALID_CONFIG with a detail for, checked in this order before the first HIP call,
 * a null idx / out, a posting-list handle (RBQ_ROTATOR_NONE), a handle without reconstruction factors (rbq_index_create),
 * null vectors, count == 0, more than 2^32 vector slots (here as far as the counts decide it, exactly once every row's list is
 * known), an unknown rescale mode, RBQ_RESCALE_CONST with ex_bits > 0 and
 * t_const <= 0, a bad device list; and, found on the device before the new arrays are allocated, first_id below the id bound,
 * a list id >= n_lists, a non-finite value in `vectors` (only when assign == NULL; with an explicit assignment there is no
 * finite check, as for the encoders).  Device failures are RBQ_DEVICE. */
int rbq_index_append(const rbq_index* idx, const float* vectors, const uint32_t* assign, uint64_t count,
                     uint64_t first_id, int rescale, float t_const, uint64_t max_chunk_rows,
                     int n_devices, const int* devices, uint32_t* out_assign, rbq_index** out);

/* 1 + the largest stored id; 0 for an index without vectors.  Found by one device reduction over the ids on first use and
 * kept in the handle. */
int rbq_index_id_bound(const rbq_index* idx, uint64_t* out);

/* TEST ONLY, process-wide: encode passes run so far (one per chunk of at most max_chunk_rows rows that rbq_index_append
 * encodes). */
uint64_t rbq_debug_append_passes(void);

/* MEASUREMENT ONLY, process-wide: device time in nanoseconds of the carry kernel of the last rbq_index_append (tools/append_rate.py
 * divides the bytes it moved by it); 0 before the first one. */
uint64_t rbq_debug_append_carry_ns(void);

#ifdef __cplusplus
}
#endif

#endif /* RBQ_APPEND_H */
