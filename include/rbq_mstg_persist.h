/*
 * rbq_mstg_persist.h — saving and loading an MSTG index in the crate's `.mstg` format (MstgIndex::save_main_index /
 * load_main_index, reference src/mstg/io.rs:129-245), assembled and taken apart on the device.  Included by rbq_mstg.h.
 *
 * The file (bincode 1.3 defaults: little-endian fixed-width integers, usize and sequence lengths as u64, enum variants as
 * u32, Option as a u8 tag, bool as u8, f32 by bit pattern):
 *   "MSTG" | u32 version = 1                                                            (not in the CRC)
 *   u64 77 | MstgConfig (src/mstg/config.rs:39-62)
 *   u64 k  | k x u32 centroid ids
 *   u64 k  | k x ( u64 len | PostingList: cluster_id u32, centroid Vec<f32>, size u32, RabitqConfig {total_bits u64,
 *            t_const Option<f32>}, vectors Vec<{vector_id u64, QuantizedVector}> )   (src/mstg/posting_list.rs:7-32)
 *   u32 CRC-32/IEEE of everything between the version word and here
 * A QuantizedVector record (src/quantizer.rs:63-88) is code Vec<u16>, binary_code_packed Vec<u8>, ex_code_packed Vec<u8>,
 * ex_bits u8, dim u64, delta, vl, f_add, f_rescale, f_error, residual_norm, f_add_ex, f_rescale_ex: with its id
 * 73 + 2 D + D / 8 + E bytes, E = D / 16 * {2, 4, 12} for ex_bits {0, 2, 6}.  A list that received no vector carries
 * RabitqConfig::default() (7, None) whatever the index's bits: PostingList::quantize_vectors returns before it sets the
 * config.
 *
 * THE HNSW SIDE FILES.  The crate also writes `{path}.hnsw.graph` and `{path}.hnsw.data` through hnsw_rs' own dump, and its
 * load_from_path requires them.  This library has no HNSW (it ranks the centroids exactly, rbq_mstg.h) and invents no graph
 * dump: it writes `{path}.mstg` only and reads `{path}.mstg` only.  A crate-written index therefore loads here; the crate
 * will not reopen a file written here unless side files of its own making lie next to it.
 */
#ifndef RBQ_MSTG_PERSIST_H
#define RBQ_MSTG_PERSIST_H

#include <stddef.h>
#include <stdint.h>

#include "rbq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MstgConfig, field for field.  metric: RBQ_METRIC_*; centroid_precision: 0 FP32, 1 BF16, 2 FP16, 3 INT8. */
typedef struct rbq_mstg_config {
    uint64_t max_posting_size;
    uint64_t branching_factor;
    float    balance_weight;
    float    closure_epsilon;
    uint64_t max_replicas;
    uint64_t rabitq_bits;
    uint8_t  faster_config;
    uint32_t metric;
    uint64_t hnsw_m;
    uint64_t hnsw_ef_construction;
    uint32_t centroid_precision;
    uint64_t default_ef_search;
    float    pruning_epsilon;
} rbq_mstg_config;

/* Writes the `.mstg` stream of an MSTG handle (rbq_mstg_build_device, rbq_mstg_load*).  The device assembles the
 * posting-list section chunk by chunk (at most 64 MB, double-buffered through page-locked memory) and computes its CRC;
 * host memory stays two chunks whatever the index size.  The stream does not depend on the chunk size.  Runs on a stream
 * of its own and only reads the index.  Centroid ids and cluster ids are 0..k-1.
 * Errors: RBQ_INVALID_CONFIG for a null argument, a handle that is no posting-list handle (its rotator is not
 * RBQ_ROTATOR_NONE), one that holds no residual norms (made by rbq_index_create*), or a cfg whose rabitq_bits or metric
 * disagree with the handle or whose enum fields are out of range; RBQ_IO when `write` returns non-zero (nothing is leaked
 * and the handle stays usable); RBQ_DEVICE. */
int rbq_mstg_save_stream(const rbq_index* idx, const rbq_mstg_config* cfg, rbq_write_fn write, void* user);

/* Whole-stream convenience: *bytes (free with rbq_persist_free_bytes) holds *len bytes. */
int rbq_mstg_save(const rbq_index* idx, const rbq_mstg_config* cfg, uint8_t** bytes, uint64_t* len);

/* (rbq_read_fn, the reader callback of the stream loaders, is declared in rbq_persist.h.) */

/* Loads a `.mstg` stream onto `device` (-1: the current device).  The framing (config, ids, list headers) is parsed on
 * the host; the records are uploaded in spans of whole lists or 32-vector blocks (at most 64 MB unless one block is larger,
 * two page-locked and two device buffers), checksummed and scattered into the device layout by the GPU, which also
 * validates every record's inner fields.  The stream form reads the framing first and the records in a second pass, so a
 * multi-GB file needs two spans of host memory; `total_len` is the length of the stream.
 * RBQ_INVALID_PERSISTENCE, with a detail string, for: a wrong magic or version; a stream that ends early or a length field
 * that runs past it; bytes after the checksum; a CRC mismatch; a config block that is not 77 bytes or holds an enum, bool or
 * Option tag out of range; rabitq_bits - 1 outside {0, 2, 6}; no list, or no vector; a centroid length that is 0, above
 * 2048, not a multiple of 16 or not the first list's; centroid ids or cluster ids that are not 0..k-1 in order (the search
 * addresses lists by position); size != vectors.len(); a non-empty list whose total_bits is not rabitq_bits or whose t_const
 * differs from the other lists'; an empty list that does not carry (7, None); a posting-list length that is not its
 * header plus its records; a record whose inner lengths, ex_bits or dim disagree with the list, whose code is not
 * ex_code + (bit << ex_bits), or (1-bit) whose ex bytes or extended factors are not zero.
 * Never aborts and never reads past a buffer.  *cfg_out receives the file's config. */
int rbq_mstg_load(const void* bytes, uint64_t len, int device, rbq_mstg_config* cfg_out, rbq_index** idx_out);
int rbq_mstg_load_stream(rbq_read_fn read, void* user, uint64_t total_len, int device, rbq_mstg_config* cfg_out,
                         rbq_index** idx_out);

/* Device bytes the handle holds on its first device (index arrays; workspaces of past searches are not counted). */
uint64_t rbq_mstg_memory_usage(const rbq_index* idx);

#ifdef __cplusplus
}
#endif

#endif /* RBQ_MSTG_PERSIST_H */
