/*
 * ivfpq_ann.h -- C ABI of the inverted-file index with product-quantised lists (`IVF<nlist>,PQ<M>` inside an id map),
 * MI355X.  The sibling of ivf_ann.h: the same coarse quantizer, lists and probed scan, with the list payload replaced by
 * M code bytes per row and the scan's inner product by a table lookup (ADC, asymmetric distance computation).
 *
 * What it replaces (paths relative to the reference's ann/src/main/):
 *   scala/com/twitter/ann/faiss/FaissIndexer.scala:82-92        index_factory(any factory string) -> train -> add_with_ids
 *   thrift/com/twitter/ann/common/ann_common.thrift:45          nprobe: "How many cells to visit in IVFPQ"
 * Not here: the decomposed "precomputed table" form, a refine index as the coarse quantizer (`quantizer_kfactor_rf`), an
 * HNSW coarse quantizer, by-id queries over this index.  The OPQ pre-transform is a layer in front of this index:
 * opq_ann.h.  Re-ranking of the answers by stored rows (`,RFlat`) is a layer around it: refine_ann.h.  Polysemous codes and
 * the search they filter (`ht`) are declared in polysemous_ann.h, over the handles of this header.
 *
 * Status codes, metric numbers, the preparation of rows, queries and centroids (fp16, Cosine L2-normalised first), the
 * distances (L2 = ||q - x||, Cosine = 1 - cos, InnerProduct = 1 - <q, x>), the tie rules, the ids rule and the clamping of
 * nprobe are those of ivf_ann.h.
 *
 * Semantics, fixed here once:
 *   Shape: M sub-quantizers of 8 bits (256 codewords each) over dsub = d / M components.  4 <= M <= 64, M % 4 == 0,
 *     d % M == 0, d a multiple of 16 and <= 512, nlist <= 65536, k <= 1024, nprobe <= 1024, n_train >= max(nlist, 256).
 *   Residuals (Faiss's by_residual = true, for all three metrics): a row's cell c is its nearest centroid by the rule of
 *     ivf_ann.h; its residual is r = fl32(x - centroid[c]), one IEEE fp32 subtraction per component of the two stored
 *     fp16 values.
 *   Codebooks: fp32 [M][256][dsub], trained after the coarse quantizer on the residuals of the training rows, one k-means
 *     per subspace, always by squared L2 whatever the metric of the index.  Deterministic Lloyd as the coarse training:
 *     the initial codewords of subspace m are the residuals of the rows mix64(seed + 0x9E3779B97F4A7C15 * (m + 1) + t)
 *     mod n_train for t = 0, 1, 2, ... (a row picked before for this subspace being skipped) until 256 are picked; niter
 *     as in ivf_index_train (0 = 20 rounds, -1 = the initial picks) and the same for both trainings; a codeword's
 *     members are summed in position order in fp64, no floating-point atomics; an empty codeword keeps its value.  Two
 *     trainings with equal arguments give byte-identical centroids and codebooks.  Faiss's own training and encoding
 *     are not vendored in the reference: parity with them is UNPINNED, exactly as the coarse training of ivf_ann.h is.
 *   Encoding: code[m] = argmin_j ||r_m - cb[m][j]||^2 evaluated in fp32, ties to the lower j.
 *   Search distance: a function of (centroids, codebooks, codes, probes, query) only, all in fp32.
 *     L2:  u = fl32(q - centroid[c]); s = sum_m ||u_m - cb[m][code_m]||^2; the distance is sqrt(s).
 *     InnerProduct / Cosine:  sim = <q, centroid[c]> + sum_m <q_m, cb[m][code_m]>; the distance is 1 - sim.
 *     A row's value comes from a fixed sequence of operations that depends neither on scheduling nor on the other
 *     queries of the batch; rows with equal codes in one cell tie exactly and come out in id order.
 *   Memory: the index keeps no copy of the rows (refine_ann.h adds one and re-ranks by it).  Per row: M code bytes in the order added, its id and its cell, and the
 *     lists, which every add lays out again device to device in (cell, id) order.
 *
 * No function throws or aborts; every function returns a status (IVF_OK, IVF_EINVAL, ... of ivf_ann.h), the message is in
 * ivfpq_last_error().  One call at a time per index.
 */
#ifndef IVFPQ_ANN_H
#define IVFPQ_ANN_H
#include <stdint.h>

#include "ivf_ann.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ivfpq_index ivfpq_index_t;

const char *ivfpq_last_error(void);

/* An empty index: nlist centroids trained on train_vectors (row-major fp32 [n_train][d]) as ivf_index_train trains them,
 * then the M codebooks on the residuals of the same rows.  niter and seed serve both trainings. */
int ivfpq_index_train(int32_t device, int32_t metric, int32_t d, int32_t nlist, int32_t M, int64_t n_train,
                      const float *train_vectors, int32_t niter, uint64_t seed, ivfpq_index_t **out);
/* The same with the centroids (row-major fp32 [nlist][d]; rounded to fp16 on the way in, Cosine normalised) and the
 * codebooks (fp32 [M][256][d / M], kept as given) supplied. */
int ivfpq_index_load(int32_t device, int32_t metric, int32_t d, int32_t nlist, int32_t M, const float *centroids,
                     const float *codebooks, ivfpq_index_t **out);
/* add_with_ids: n rows (row-major fp32 [n][d]) are assigned, encoded and put in their lists.  ids as in ivf_index_add. */
int ivfpq_index_add(ivfpq_index_t *index, int64_t n, const float *vectors, const int64_t *ids);
/* As ivf_search, over the codes: out_dist[nq*k], out_ids[nq*k] ascending by (distance, id), out_counts[nq] <= k. */
int ivfpq_search(ivfpq_index_t *index, int32_t nq, const float *queries, int32_t k, int32_t nprobe, float *out_dist,
                 int64_t *out_ids, int32_t *out_counts);

/* Rows, dimension, metric, number of cells and of sub-quantizers (any pointer may be NULL). */
int ivfpq_index_info(const ivfpq_index_t *index, int64_t *n, int32_t *d, int32_t *metric, int32_t *nlist, int32_t *M);
/* The stored (fp16-rounded, for Cosine normalised) centroids as fp32 [nlist][d]. */
int ivfpq_index_get_centroids(const ivfpq_index_t *index, float *out);
/* The codebooks: fp32 [M][256][d / M]. */
int ivfpq_index_get_codebooks(const ivfpq_index_t *index, float *out);
/* The codes of the rows in the order they were added: uint8 [n][M]. */
int ivfpq_index_get_codes(const ivfpq_index_t *index, uint8_t *out);
/* Rows per cell: int64 [nlist]. */
int ivfpq_index_list_sizes(const ivfpq_index_t *index, int64_t *out);
/* For every row in the order it was added: its id and its cell ([n] each; either may be NULL). */
int ivfpq_index_get_assignment(const ivfpq_index_t *index, int64_t *out_ids, int32_t *out_cells);
/* As ivf_last_probes. */
int ivfpq_last_probes(const ivfpq_index_t *index, int32_t *nq, int32_t *nprobe, int32_t *out_cells);
/* As ivf_last_stats: rows scanned, scan rounds (1 + fallback rounds of the 8192-survivor buffer), HIP-event milliseconds. */
int ivfpq_last_stats(const ivfpq_index_t *index, int64_t *rows_scanned, int32_t *rounds, float *coarse_ms, float *scan_ms,
                     float *select_ms);
int ivfpq_index_destroy(ivfpq_index_t *index);

#ifdef __cplusplus
}
#endif
#endif
