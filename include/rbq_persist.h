/*
 * rbq_persist.h — saving a device-resident IVF index in the crate's RBQ1 v3 format (IvfRabitqIndex::save_to_writer,
 * reference src/ivf.rs:1310-1474), and creating one with the per-vector reconstruction factors RBQ1 stores.
 * Included by rbq.h; kept in a header of its own so that rbq.h stays the boundary integration/gpu_ivf.rs binds.
 */
#ifndef RBQ_PERSIST_H
#define RBQ_PERSIST_H

#include <stddef.h>
#include <stdint.h>

#include "rbq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rbq_index_create with the reconstruction factors of every list: delta[c] and vl[c] point to list c's n f32 each (RBQ1's
 * `delta` / `vl`, reference src/quantizer.rs:172-187; search never reads them).  A handle made by rbq_index_create has none
 * and cannot be saved.  rbq_index_load_rbq1 and the device encoders (rbq_index_build_device*, rbq_build_stream_*) keep them
 * themselves.  The factors live on the first device only (8 bytes per vector). */
int rbq_index_create_with_recon(const rbq_header* hdr, const rbq_list_view* lists, const float* const* delta,
                                const float* const* vl, int n_devices, const int* devices, rbq_index** out);

/* Receives the stream in order, piece by piece; returns 0 to go on, anything else to stop the save (-> RBQ_IO). */
typedef int (*rbq_write_fn)(void* user, const void* bytes, uint64_t len);

/* Writes the index as the bytes of save_to_writer: header, rotator, every cluster, CRC-32.  The device assembles the
 * cluster bytes chunk by chunk (at most 64 MB, double-buffered through page-locked memory) and computes their CRC; host
 * memory stays two chunks plus the header and rotator, whatever the index size.  Runs on a stream of its own and only
 * reads the index: searches on other threads may run meanwhile.  A multi-device handle saves from its first device.
 * Errors: RBQ_INVALID_CONFIG for a handle without reconstruction factors (rbq_index_create) or a posting-list handle
 * (RBQ_ROTATOR_NONE: the crate has no tag for it); RBQ_IO when `write` returns non-zero (nothing is leaked and the handle
 * stays usable); RBQ_DEVICE.  Like the crate, clusters above the crate loader's 1 M-vector cap are written as they are;
 * the crate (and rbq_index_load_rbq1) will refuse such a file. */
int rbq_index_save_rbq1_stream(const rbq_index* idx, rbq_write_fn write, void* user);

/* Whole-stream convenience: *bytes (free with rbq_persist_free_bytes) holds *len bytes. */
int rbq_index_save_rbq1(const rbq_index* idx, uint8_t** bytes, uint64_t* len);
void rbq_persist_free_bytes(uint8_t* bytes);

/* Test hook: CRC-32/IEEE of `len` device bytes at `d_bytes` (any alignment) on `device`, with the save path's kernels. */
int rbq_debug_crc32_device(const void* d_bytes, uint64_t len, int device, uint32_t* out);

#ifdef __cplusplus
}
#endif

#endif /* RBQ_PERSIST_H */
