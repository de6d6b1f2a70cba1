/* rbq_build.h — C ABI of the CPU index builder (train-time harness; see rbq_build.cpp). */
#ifndef RBQ_BUILD_H
#define RBQ_BUILD_H
#include <stdint.h>
#include "../../../include/rbq.h"
#include "../../../include/rbq_mstg_persist.h" /* rbq_mstg_config */
#ifdef __cplusplus
extern "C" {
#endif
typedef struct rbq_built rbq_built;

/* IvfRabitqIndex::train_with_clusters (reference src/ivf.rs:1025-1103). centroids are in the
 * ORIGINAL space ([nlist][dim]); data [n][dim]; assignments [n] < nlist. */
int rbq_build_train_with_clusters(const float* data, uint64_t n, uint32_t dim,
                                  const float* centroids, uint64_t nlist, const uint32_t* assignments,
                                  uint32_t total_bits, uint8_t metric, uint8_t rotator_type,
                                  uint64_t seed, int use_faster_config, rbq_built** out);
const rbq_header*    rbq_built_header(const rbq_built* b);
const rbq_list_view* rbq_built_lists(const rbq_built* b);
float                rbq_built_t_const(const rbq_built* b);
/* ClusterData.delta / .vl of list c (persisted by save_to_writer, unused by search: not part of rbq_list_view), and
 * QuantizedVector::residual_norm of its vectors (kept by the `.mstg` format); [n] each, owned by b.
 * RBQ_INVALID_CONFIG: a null pointer or c >= n_lists. */
int rbq_built_list_recon(const rbq_built* b, uint64_t c, const float** delta, const float** vl);
int rbq_built_list_residual_norm(const rbq_built* b, uint64_t c, const float** rnorm);
void                 rbq_built_free(rbq_built* b);
/* IvfRabitqIndex::save_to_writer (src/ivf.rs:1317-1474) into a malloc'd buffer. */
int  rbq_built_save_rbq1(const rbq_built* b, uint8_t** bytes, uint64_t* len);
void rbq_build_free_bytes(uint8_t* p);
/* The `.mstg` loader's whole validation without a GPU (rbq_mstg_file.hpp): framing, every record's inner fields, the checksum.
 * Returns the loader's code with its message in detail [detail_cap]; cfg_out (nullable) receives the file's config, out4
 * (nullable) lists, vectors, dim, ex_bits. */
int rbq_build_mstg_file_check(const void* bytes, uint64_t len, char* detail, uint64_t detail_cap, rbq_mstg_config* cfg_out,
                              uint64_t* out4);

/* best_rescale_factor (src/quantizer.rs:337-427) of one vector: o_abs [dim] = |r_i| / norm(r) -> t */
double rbq_build_best_rescale_factor(const float* o_abs, uint64_t dim, uint32_t ex_bits);
void rbq_build_pack_binary_code(const uint8_t* bits, uint8_t* packed, uint64_t dim);
void rbq_build_pack_ex_code_1bit(const uint16_t* c, uint8_t* p, uint64_t dim);
void rbq_build_pack_ex_code_2bit(const uint16_t* c, uint8_t* p, uint64_t dim);
void rbq_build_pack_ex_code_6bit(const uint16_t* c, uint8_t* p, uint64_t dim);
void rbq_build_pack_codes(const uint8_t* codes, uint64_t num_vectors, uint64_t dim_bytes, uint8_t* packed);
uint32_t rbq_build_crc32(const uint8_t* p, uint64_t n);
void rbq_build_rotate(const rbq_header* h, const float* in, float* out);
int  rbq_build_kmeans(const float* data, uint64_t n, uint32_t dim, uint64_t k, int iters, uint64_t seed,
                      float* centroids, uint32_t* assignments);
/* run_kmeans_with_config (reference src/kmeans.rs) in the pinned arithmetic of rbq_build.cpp: the specification of the GPU
 * k-means (rbq_kmeans_device).  data [n][dim] (finite); centroids [k][dim], assignments [n], objective.  stats (nullable) [2]:
 * empty clusters reseeded, reseeds drawn from the RNG (summed over restarts).  RBQ_INVALID_CONFIG: n == 0, k == 0, k > n,
 * niter == 0, nredo == 0, decode_block_size == 0, dim == 0, n >= 2^32 - 1 or a non-finite value. */
int  rbq_build_kmeans_faiss(const float* data, uint64_t n, uint32_t dim, uint64_t k, uint64_t niter, uint64_t nredo, uint64_t seed,
                            int spherical, uint64_t max_points_per_centroid, uint64_t decode_block_size, float* centroids,
                            uint32_t* assignments, double* objective, uint64_t* stats);

/* BruteForceRabitqIndex::train (reference src/brute_force.rs:214-287): data [n][dim]; every vector quantised against a
 * zero centroid.  total_bits 1, 3 or 7; rotator MATRIX or FHT_KAC.  The view's ex_len is padded_dim/8 for 1-bit indexes
 * (the zero bytes the crate's quantiser leaves in ex_code_packed). */
typedef struct rbq_bf_built rbq_bf_built;
int rbq_build_train_bruteforce(const float* data, uint64_t n, uint32_t dim, uint32_t total_bits, uint8_t metric,
                               uint8_t rotator_type, uint64_t seed, int use_faster_config, rbq_bf_built** out);
const rbq_header*  rbq_bf_built_header(const rbq_bf_built* b);
const rbq_bf_view* rbq_bf_built_view(const rbq_bf_built* b);
float              rbq_bf_built_t_const(const rbq_bf_built* b); /* the faster config's constant rescale factor (0: not used) */
void               rbq_bf_built_free(rbq_bf_built* b);

/* ClosureAssigner::assign (reference src/mstg/closure.rs:24-107) for every row of data [n][dim] against centroids
 * [n_lists][dim]: the parity yardstick of rbq_mstg_closure_assign (include/rbq_mstg.h), OpenMP over the rows.  Distances
 * are math::l2_distance_sqr in its AVX2 order; the sort is stable (equal distances keep ascending centroid index).
 * out_lists [n][max_replicas] (unused slots UINT32_MAX, the crate's Vec order), out_counts [n].
 * RBQ_INVALID_CONFIG: a null pointer, n == 0, n_lists == 0, dim == 0, max_replicas == 0, epsilon negative or not finite
 * (the crate panics on the last two).  Non-finite data is not checked: the result is then unspecified. */
int rbq_build_closure_assign(const float* centroids, uint64_t n_lists, uint32_t dim, const float* data, uint64_t n,
                             float epsilon, uint32_t max_replicas, uint32_t* out_lists, uint32_t* out_counts);

/* The list selection of MstgIndex::search as rbq_mstg_search_batch defines it (include/rbq_mstg.h, "the selection"): for
 * every query the min(ef_search, n_lists) nearest centroids under (bits of math::l2_distance_sqr in its AVX2 order,
 * centroid index), cut where sqrtf(distance) > sqrtf(closest) * (1.0f + pruning_epsilon).  The parity yardstick of the
 * device selection, OpenMP over the queries.  out_lists [nq][min(ef_search, n_lists)] in scan order (unused slots
 * UINT32_MAX), out_counts [nq].  Any pruning_epsilon is taken; a query with a NaN distance, or whose closest distance is
 * +inf, selects nothing.  RBQ_INVALID_CONFIG: a null pointer, n_lists == 0 or >= 2^32 - 1, dim == 0. */
int rbq_build_mstg_select_lists(const float* centroids, uint64_t n_lists, uint32_t dim, const float* queries, uint64_t nq,
                                uint32_t ef_search, float pruning_epsilon, uint32_t* out_lists, uint32_t* out_counts);

/* HierarchicalClustering{max_cluster_size, branching_factor, balance_weight, max_iterations}.cluster(data) (reference
 * src/mstg/clustering.rs), step 1 of MstgIndex::build, in the pinned arithmetic stated in rbq_hcluster.hpp: the specification
 * of rbq_mstg_cluster_device (include/rbq_mstg.h), which equals it bit for bit.  data [n][dim], finite.  The handle holds the
 * final clusters in the crate's pop order: centroids [count][dim], offsets [count + 1], members [n] (row indices, cluster by
 * cluster, each in its own order) and stats [6]: splits, balance moves, empty clusters reseeded, reseeds drawn from the RNG,
 * host splits (0 here) and arena bytes (0 here).
 * RBQ_INVALID_CONFIG, with a static message in *detail (nullable): a null pointer, n == 0, dim == 0, n >= 2^32 - 1,
 * max_iterations == 0, branching_factor < 2 or > max_posting_size + 1, a non-finite value; and, found while running, a split
 * that leaves a single non-empty subcluster (the crate would loop for ever).  Any balance_weight is taken: NaN or <= 0 means
 * no balancing. */
typedef struct rbq_hclustered rbq_hclustered;
int rbq_build_hcluster(const float* data, uint64_t n, uint32_t dim, uint64_t max_posting_size, uint64_t branching_factor,
                       float balance_weight, uint64_t max_iterations, rbq_hclustered** out, const char** detail);
uint64_t        rbq_hclustered_count(const rbq_hclustered* h);
const float*    rbq_hclustered_centroids(const rbq_hclustered* h);
const uint64_t* rbq_hclustered_offsets(const rbq_hclustered* h);
const uint32_t* rbq_hclustered_members(const rbq_hclustered* h);
const uint64_t* rbq_hclustered_stats(const rbq_hclustered* h);
void            rbq_hclustered_free(rbq_hclustered* h);
#ifdef __cplusplus
}
#endif
#endif
