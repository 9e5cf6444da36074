/*
 * ivf_ann.h -- C ABI of the inverted-file index with flat lists (`IVF<nlist>,Flat` inside an id map), MI355X.
 *
 * Replaces the reference's third dense `Queryable`, the Faiss one (all paths relative to the reference's ann/src/main/):
 *   scala/com/twitter/ann/faiss/FaissIndexer.scala:82-92        index_factory -> train(first trainingSetSize rows)
 *                                                               -> add_with_ids(all)
 *   scala/com/twitter/ann/faiss/FaissIndexer.scala:44-50        Cosine: rows are L2-normalised, then InnerProduct
 *   scala/com/twitter/ann/faiss/QueryableIndexAdapter.scala:139-178   queryWithDistance over Index.search
 *   thrift/com/twitter/ann/common/ann_common.thrift:41-56       FaissRuntimeParam: nprobe first
 *   thrift/com/twitter/ann/common/ann_common.thrift:16-19       enum DistanceMetric { L2, Cosine, InnerProduct }
 * Only the coarse quantizer, its training, the inverted lists and the probed scan are here.  Product quantisation
 * (codebooks, ADC tables) replaces the list payload and the scan's inner product, nothing else: that index is
 * ivfpq_ann.h.  `quantizer_kfactor_rf` (a refine index as the coarse quantizer) is in neither; `ht` (polysemous codes over
 * the product-quantised lists) is polysemous_ann.h; top-level refinement of the product-quantised answers by stored rows
 * is refine_ann.h.
 *
 * Arithmetic: as in dense_ann.h.  Rows, queries and centroids are rounded to fp16 (Cosine: L2-normalised first, the
 * index then behaves as InnerProduct), products accumulate in fp32 on the matrix cores.  Distances are those of
 * dense_ann.h (L2 = ||q - x||, Cosine = 1 - cos, InnerProduct = 1 - <q, x>), so answers of the three indexes are
 * comparable and dann_compose_shards composes them.
 *
 * Semantics, fixed here once:
 *   Assignment and probing use the metric of the index: L2 nearest by ||x - c||; InnerProduct and Cosine largest <x, c>
 *     (as Faiss's IndexFlatIP quantizer does).  Ties go to the lower cell number.
 *   Training is Lloyd's k-means and deterministic: two calls with the same arguments give byte-identical centroids.
 *     Initial centroids are the training rows mix64(seed + t) mod n_train for t = 0, 1, 2, ... (mix64: the 64-bit
 *     finaliser of sann_device.h), a row picked before being skipped, until nlist rows are picked.  Then `niter` rounds
 *     of assign -> mean: niter = 0 means 20 rounds, niter = -1 means none (the initial picks are the centroids).  A cell
 *     that received no row keeps its centroid.  A cell's rows are summed in position order in fp64 by one thread per
 *     component: no floating-point atomics.  For InnerProduct and Cosine the mean is re-normalised to unit length
 *     (spherical k-means), and so are the initial picks of an InnerProduct index (Cosine rows are unit length already):
 *     every round then lowers the mean of 1 - <x, c> over unit centroids.  Faiss's own training (random subsampling,
 *     cluster splitting) is not vendored in the reference, whose native binary is absent: parity with it is UNPINNED,
 *     exactly as the dense arithmetic is.
 *   ivf_search's nprobe above nlist is clamped to nlist, as Faiss does; ivf_last_probes reports the clamped width.
 *
 * No function throws or aborts; every function returns a status, the message is in ivf_last_error().
 * One call at a time per index.
 */
#ifndef IVF_ANN_H
#define IVF_ANN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define IVF_OK 0
#define IVF_EINVAL 1
#define IVF_EDEVICE 2
#define IVF_ELIMIT 3
#define IVF_ENOMEM 4    /* host allocation failed */
#define IVF_EINTERNAL 5 /* an unexpected C++ exception was caught at the ABI; the message says which */

/* ann_common.thrift:16-19 */
#define IVF_METRIC_L2 0
#define IVF_METRIC_COSINE 1
#define IVF_METRIC_INNER_PRODUCT 2

typedef struct ivf_index ivf_index_t;

const char *ivf_last_error(void);

/* An empty index whose nlist centroids are trained on train_vectors (row-major fp32 [n_train][d]).  d a multiple of 16
 * and <= 512; 1 <= nlist <= 65536; n_train >= nlist; niter >= -1 (0 = 20 rounds, -1 = the initial picks). */
int ivf_index_train(int32_t device, int32_t metric, int32_t d, int32_t nlist, int64_t n_train, const float *train_vectors,
                    int32_t niter, uint64_t seed, ivf_index_t **out);
/* The same with the centroids given (row-major fp32 [nlist][d]; rounded to fp16 on the way in, Cosine normalised). */
int ivf_index_load(int32_t device, int32_t metric, int32_t d, int32_t nlist, const float *centroids, ivf_index_t **out);
/* add_with_ids: n rows (row-major fp32 [n][d]) are each put in the list of their nearest centroid.  ids: n of them, or
 * NULL (ids = positions in the order added); every call on one index gives ids, or none does (else IVF_EINVAL, index
 * unchanged).  May be called more than once; every call lays all lists out again, device to device, in (cell, id)
 * order.  Nothing but sizes leaves the device. */
int ivf_index_add(ivf_index_t *index, int64_t n, const float *vectors, const int64_t *ids);
/* nq queries (row-major fp32 [nq][d]): for each, the nprobe nearest cells, then the k nearest rows among those cells'
 * lists, ascending by (distance, id): out_dist[nq*k], out_ids[nq*k], out_counts[nq] <= k (the probed lists may hold
 * fewer than k rows; where Faiss pads with label -1 this reports the count).  k <= 1024, 1 <= nprobe <= 1024; nprobe
 * above nlist is clamped to nlist.  Exact over the probed lists. */
int ivf_search(ivf_index_t *index, int32_t nq, const float *queries, int32_t k, int32_t nprobe, float *out_dist,
               int64_t *out_ids, int32_t *out_counts);

/* Rows, dimension, metric and number of cells (any pointer may be NULL). */
int ivf_index_info(const ivf_index_t *index, int64_t *n, int32_t *d, int32_t *metric, int32_t *nlist);
/* The stored (fp16-rounded, for Cosine normalised) centroids as fp32 [nlist][d]. */
int ivf_index_get_centroids(const ivf_index_t *index, float *out);
/* Rows per cell: int64 [nlist]. */
int ivf_index_list_sizes(const ivf_index_t *index, int64_t *out);
/* For every row in the order it was added: its id and its cell ([n] each; either may be NULL). */
int ivf_index_get_assignment(const ivf_index_t *index, int64_t *out_ids, int32_t *out_cells);
/* The cells the last ivf_search probed, nearest first: int32 [nq][nprobe] with the shape in *nq / *nprobe (nprobe
 * after clamping).  out_cells NULL asks for the shape alone. */
int ivf_last_probes(const ivf_index_t *index, int32_t *nq, int32_t *nprobe, int32_t *out_cells);
/* Of the last ivf_search: rows scanned = the sum over queries of the sizes of their probed lists; scan rounds = 1, plus
 * one per fallback round in which some query's probed lists held more candidates than its survivor buffer (8192) and
 * it was scanned again above a threshold; HIP-event milliseconds of the coarse search, the scan rounds and the
 * selection (any pointer may be NULL). */
int ivf_last_stats(const ivf_index_t *index, int64_t *rows_scanned, int32_t *rounds, float *coarse_ms, float *scan_ms,
                   float *select_ms);
int ivf_index_destroy(ivf_index_t *index);

#ifdef __cplusplus
}
#endif
#endif
