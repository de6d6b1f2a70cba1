/*
 * rbq_kmeans.h — C ABI of the device k-means: lqhl/rabitq-rs's `run_kmeans_with_config` (reference src/kmeans.rs), the
 * clustering step of `IvfRabitqIndex::train`.  Included by rbq.h; kept in a header of its own, like rbq_bf.h.
 *
 * The arithmetic is pinned: the result equals, bit for bit, the CPU restatement
 * rbq_build_kmeans_faiss of the project's builder: centroids, assignments and objective.  It is the crate's algorithm step by
 * step (sampling, Forgy, Lloyd iterations, reseeding of empty clusters, final assignment of every row, objective, restarts),
 * not its exact numbers: the crate merges Rayon partial sums in scheduling order, takes dot products from an sgemm and draws
 * from ChaCha12.
 */
#ifndef RBQ_KMEANS_H
#define RBQ_KMEANS_H

#include <stddef.h>
#include <stdint.h>

#include "rbq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* k-means of d_data [n][dim] (f32, DEVICE pointer on `device`) into k clusters.  The config fields are KMeansConfig's
 * (src/kmeans.rs:13-37; the crate's defaults: niter 25, nredo 1, seed 42, spherical 0, max_points_per_centroid 256,
 * decode_block_size 32768).
 * Outputs: centroids [k][dim] f32 (HOST), d_assignments [n] u32 (DEVICE, the layout rbq_index_build_device_ex takes),
 * *objective.  stats (HOST, nullable) [4]: rows whose approximate shortlist overflowed and were scored exactly against every
 * cluster, empty clusters reseeded, reseeds drawn from the RNG, largest shortlist seen.
 * RBQ_INVALID_CONFIG (detail from rbq_last_error_detail): n == 0, k == 0, k > n, niter == 0, nredo == 0,
 * decode_block_size == 0, dim == 0, n >= 2^32 - 1, or a non-finite input value (the crate does not check; the error bound of
 * the approximate assignment needs finite input).
 * Device workspace beyond the data: the training sample when one is drawn, O(n + k * dim) arrays and the chunked assignment
 * workspace of at most max(512 MiB, 128 * (4k + 4 dim + 1156)) bytes. */
int rbq_kmeans_device(const float* d_data, uint64_t n, uint32_t dim, uint64_t k, uint64_t niter, uint64_t nredo, uint64_t seed,
                      int spherical, uint64_t max_points_per_centroid, uint64_t decode_block_size, int device, float* centroids,
                      uint32_t* d_assignments, double* objective, uint64_t* stats);

/* TEST ONLY, process-wide: at most `rows` rows per pass of the chunked assignment (rounded down to a multiple of 128, at
 * least 128); returns the previous value (0: the default, by the 512 MiB workspace, which 0 also restores).  It applies to
 * rbq_kmeans_device and to the splits of rbq_mstg_cluster_device above 256 subclusters, read when a call sizes its
 * workspace; the closure assignment keeps its own max_chunk_rows.  Results and stats do not depend on it. */
uint64_t rbq_debug_set_kmeans_chunk_rows(uint64_t rows);
/* TEST ONLY, process-wide: passes of the chunked assignment run so far (one per chunk of rows per assignment). */
uint64_t rbq_debug_kmeans_assign_passes(void);
/* TEST ONLY: the front that k-means, the hierarchical splits, rbq_index_append's nearest list, the MSTG closure assignment and
 * the MSTG list selection share, alone, through the launchers those drivers call: canonical norms, split-bf16 images padded
 * with zeros to Dp = dim rounded up to 32, and the ranking GEMM's approximate inner products.  centroids [k][dim] and rows
 * [n][dim] are HOST pointers (k >= 1, dim >= 1, any n); a non-finite value is RBQ_INVALID_CONFIG, as in the drivers.  Rows go
 * through in passes of the chunked assignment's size (rbq_debug_set_kmeans_chunk_rows applies), every pass reusing one set of
 * buffers.  Outputs (HOST): out_dots [n][k] f32, out_nx [n] f32, out_nc [k] f32, *out_ncmax (the largest of out_nc);
 * out_row_hi / out_row_lo [n][Dp] u16 and out_cent_hi / out_cent_lo [k][Dp] u16, each pair NULL or given. */
int rbq_debug_gemm_shortlist_front(const float* centroids, uint64_t k, uint32_t dim, const float* rows, uint64_t n, int device,
                                   float* out_dots, float* out_nx, float* out_nc, float* out_ncmax, uint16_t* out_row_hi,
                                   uint16_t* out_row_lo, uint16_t* out_cent_hi, uint16_t* out_cent_lo);

#ifdef __cplusplus
}
#endif

#endif /* RBQ_KMEANS_H */
