/*
 * ivfsq_ann.h -- C ABI of the inverted-file index with 8-bit scalar-quantised lists (`IVF<nlist>,SQ8` inside an id map),
 * MI355X.
 *
 * The reference hands any Faiss factory string to index_factory (all paths relative to the reference's ann/src/main/):
 *   scala/com/twitter/ann/faiss/FaissIndexer.scala:82-92        index_factory -> train(first trainingSetSize rows)
 *                                                               -> add_with_ids(all)
 *   scala/com/twitter/ann/faiss/FaissIndexer.scala:44-50        Cosine: rows are L2-normalised, then InnerProduct
 *   scala/com/twitter/ann/dataflow/offline/ANNIndexBuilderBeamJob.scala:143-144
 *                                                               the string "determines the ANN algorithm and compression"
 *   scala/com/twitter/ann/faiss/QueryableIndexAdapter.scala:139-178   queryWithDistance over Index.search
 *   thrift/com/twitter/ann/common/ann_common.thrift:41-56       FaissRuntimeParam: nprobe first
 * `IVF<nlist>,SQ8` stands between `IVF<nlist>,Flat` (ivf_ann.h: fp16 rows, 2 d bytes per row and copy) and
 * `IVF<nlist>,PQ<M>` (ivfpq_ann.h: M bytes per row): one byte per component, distances close to the flat ones.
 *
 * Semantics, fixed here once.
 *
 * Coarse quantizer, assignment, probing: everything is ivf_ann.h's -- the metrics, the tie rules, the clamping of nprobe,
 *   ids on every add or on none, (distance, id) order of the answers.  ivfsq_index_train obtains its centroids as
 *   ivfpq_index_train does, from ivf_index_train: equal arguments give the centroids of ivf_index_train byte for byte.
 *   Shape limits are the family's: d a multiple of 16 in 16..512, nlist in 1..65536, n_train >= nlist, k <= 1024, nprobe
 *   in 1..1024.
 *
 * Ranges (Faiss's QT_8bit: per component, range statistic min/max with argument 0).  Over all n_train prepared training
 *   rows (fp16 values, Cosine rows normalised first, as every index of the family prepares rows):
 *     vmin[i] = the minimum, vmax[i] = the maximum of component i (a zero is +0),
 *     vdiff[i] = fl32(vmax[i] - vmin[i]),   step[i] = fl32(vdiff[i] / 255).
 *   Minimum and maximum are exact and independent of any order (integer atomics on an order-preserving key; no
 *   floating-point atomics).  A training set with a non-finite prepared value is refused.
 *
 * Code.  The code of component i of a prepared row x is
 *     clamp(floor(fl32(fl32(x[i] - vmin[i]) / step[i])), 0, 255),
 *   the subtraction and the division single IEEE fp32 operations (no contraction, correctly rounded division).  A
 *   component with step[i] == 0 has code 0.  Rows outside the trained range clip.
 *
 * Stored row.  xhat[i] = vmin[i] + (code[i] + 0.5) step[i], as a real number of the fp32 parameters.
 *
 * The index's inner product of a prepared query q (fp16 values) with a stored row:
 *     P(q, row) = b_q + sum_i s[i] code[i],
 *     s[i] = fp16(fl32(q[i] step[i])),
 *     b_q  = fl32(sum_i q[i] (vmin[i] + step[i] / 2)), summed in fp64.
 *   The sum over i runs on the matrix cores with fp32 accumulation.  The rounding of s to fp16 is part of the contract: it
 *   is of the size of the rounding of q to fp16 that every index here applies already, and it is what lets the list bytes
 *   go to the MFMA as exact integers (0..255 are fp16 values).
 *
 * Score and distance.  score = (bias_row + sum_i s[i] code[i]) + b_q, where bias_row is 0 for InnerProduct and Cosine,
 *   -|xhat|^2 / 2 for L2 (|xhat|^2 summed in fp64 at add time and rounded once to fp32) and -inf in the padding of a
 *   list's last block.  The distance is that of the flat index's select step, unchanged: L2 sqrt(max(0, |q|^2 - 2 score))
 *   with the sum of squares of the prepared query, otherwise 1 - score.
 *
 * What the index keeps per row: in the order added d code bytes, |xhat|^2 (4), the cell (4) and the id (8); in the lists
 *   d code bytes, the bias (4) and the rank (4), beside the id in sorted order (8): 2 d + 32 bytes per row, the padding of
 *   a list's last 32-row block aside.  The fp16 rows of an add live only in its staging slab.  (IVF-Flat: 4 d + 32.)
 *
 * UNPINNED: parity with Faiss, as everywhere in this family (Faiss is not vendored in the reference).  One deliberate
 *   difference is named: the code is of the row itself (by_residual = false), not of the residual to its centroid.  With
 *   it, one range and one scaled query serve a whole search.  Residual coding is a later change.
 *
 * Out of scope: residual coding; the other quantiser types (SQ4, SQ6, SQfp16, the uniform and direct ones); a flat SQ8
 *   without IVF; `,RFlat` over this index; an attached HNSW quantizer; ShardSet membership and the device-output search;
 *   saving and loading (no FAISS_KIND); by-id queries; JNI.
 *
 * Status codes are the IVF_* numbers of ivf_ann.h.  No function throws or aborts; every function returns a status, the
 * message is in ivfsq_last_error().  One call at a time per index.
 */
#ifndef IVFSQ_ANN_H
#define IVFSQ_ANN_H
#include <stdint.h>

#include "ivf_ann.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ivfsq_index ivfsq_index_t;

const char *ivfsq_last_error(void);

/* An empty index: the centroids of ivf_index_train over the same arguments, and the ranges of the prepared training rows. */
int ivfsq_index_train(int32_t device, int32_t metric, int32_t d, int32_t nlist, int64_t n_train, const float *train_vectors,
                      int32_t niter, uint64_t seed, ivfsq_index_t **out);
/* The same with the centroids (row-major fp32 [nlist][d], as ivf_index_load takes them) and the ranges given: vmin and vdiff
 * fp32 [d].  A non-finite value or a negative vdiff is refused. */
int ivfsq_index_load(int32_t device, int32_t metric, int32_t d, int32_t nlist, const float *centroids, const float *vmin,
                     const float *vdiff, ivfsq_index_t **out);
/* add_with_ids, as ivf_index_add: the rows are prepared, assigned to their nearest centroid and encoded. */
int ivfsq_index_add(ivfsq_index_t *index, int64_t n, const float *vectors, const int64_t *ids);
/* As ivf_search, over the stored rows xhat: exact over the probed lists in the arithmetic stated above. */
int ivfsq_search(ivfsq_index_t *index, int32_t nq, const float *queries, int32_t k, int32_t nprobe, float *out_dist,
                 int64_t *out_ids, int32_t *out_counts);

/* Rows, dimension, metric and number of cells (any pointer may be NULL). */
int ivfsq_index_info(const ivfsq_index_t *index, int64_t *n, int32_t *d, int32_t *metric, int32_t *nlist);
/* The stored centroids as fp32 [nlist][d]. */
int ivfsq_index_get_centroids(const ivfsq_index_t *index, float *out);
/* vmin and vdiff, fp32 [d] each (either may be NULL). */
int ivfsq_index_get_ranges(const ivfsq_index_t *index, float *vmin, float *vdiff);
/* Rows per cell: int64 [nlist]. */
int ivfsq_index_list_sizes(const ivfsq_index_t *index, int64_t *out);
/* For every row in the order it was added: its id and its cell ([n] each; either may be NULL). */
int ivfsq_index_get_assignment(const ivfsq_index_t *index, int64_t *out_ids, int32_t *out_cells);
/* The codes of rows [r0, r0 + m) in the order added: uint8 [m][d]. */
int ivfsq_index_get_codes(const ivfsq_index_t *index, int64_t r0, int64_t m, uint8_t *out);
/* As ivf_last_probes. */
int ivfsq_last_probes(const ivfsq_index_t *index, int32_t *nq, int32_t *nprobe, int32_t *out_cells);
/* As ivf_last_stats. */
int ivfsq_last_stats(const ivfsq_index_t *index, int64_t *rows_scanned, int32_t *rounds, float *coarse_ms, float *scan_ms,
                     float *select_ms);
int ivfsq_index_destroy(ivfsq_index_t *index);

#ifdef __cplusplus
}
#endif
#endif
