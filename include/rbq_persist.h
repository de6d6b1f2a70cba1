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

/* Reads `len` bytes at stream offset `offset` into dst; returns 0, or anything else when the range cannot be read. */
typedef int (*rbq_read_fn)(void* user, uint64_t offset, void* dst, uint64_t len);

/* rbq_index_load_rbq1 over a reader: the same handle, bit for bit, and the same errors (code and rbq_last_error_detail) as
 * rbq_index_load_rbq1 gives for the same `total_len` bytes, without the stream ever lying in host memory as a whole.
 * A framing pass on the host reads the header, the rotator and, per cluster, the two fields that fix its layout (the
 * vector count and batch_data's length).  The cluster region is then read in spans of at most 64 MB cut at field
 * boundaries (whole batch records, whole length-prefixed ex codes, whole ids, whole f32s: a span may end inside a list and
 * inside any of its sections); the read of span i + 1 overlaps the kernels on span i.  The GPU checksums every span
 * (the span CRCs are combined with the host CRC of header and rotator), checks every ex-code length prefix and scatters
 * the span into the device layout.  Host memory: two page-locked spans, their piece tables and 12 bytes per list.
 * `read` is called on the calling thread only, for ranges inside [0, total_len) of at most one span each; a non-zero
 * return is RBQ_IO "read callback failed".  A null `read` or `out` is RBQ_INVALID_CONFIG.  *out is null after any error
 * and nothing is leaked.  Bytes after the checksum are ignored. */
int rbq_index_load_rbq1_stream(rbq_read_fn read, void* user, uint64_t total_len, int n_devices, const int* devices,
                               rbq_index** out);

/* Test hook, process-wide: the span size of rbq_index_load_rbq1_stream in bytes; returns the previous value (0: the 64 MB
 * default, which 0 also restores).  A value below the largest indivisible unit of the stream being loaded (one batch
 * record) is raised to that unit; one above 1 GiB is lowered to 1 GiB.  The loaded index does not depend on it. */
uint64_t rbq_debug_set_load_span(uint64_t bytes);

#ifdef __cplusplus
}
#endif

#endif /* RBQ_PERSIST_H */
