/*
 * opq_ann.h -- C ABI of the OPQ pre-transform in front of the IVF-PQ index (`OPQ<M>[_<dout>],IVF<nlist>,PQ<M>` inside
 * an id map), MI355X.  A learned matrix with orthonormal rows (Faiss's OPQMatrix inside an IndexPreTransform) rotates
 * and, with d_out < d_in, projects every row and query before the index of ivfpq_ann.h sees it.
 *
 * What it replaces (paths relative to the reference's ann/src/main/):
 *   python/dataflow/faiss_index_bq_dataset.py:178-188           the factory string built when the caller gives none:
 *                                                               OPQ<M>_<dout>,IVF<nlist>,PQ<M> with M = 48,
 *                                                               dout = (d / M) M, nlist = N / 20
 *   scala/com/twitter/ann/faiss/FaissIndexer.scala:82-92        index_factory(any factory string) -> train -> add_with_ids
 *   scala/com/twitter/ann/faiss/QueryableIndexAdapter.scala:43-65   Cosine: normalise, search by inner product, 1 - sim
 * Not here: a refine index as the coarse quantizer (`quantizer_kfactor_rf`), an HNSW coarse quantizer, by-id queries
 * over this index, OPQ with a number of sub-quantizers other than the index's M.  Top-level refinement (`,RFlat`: the
 * answers re-ranked by the stored rows, before the transform) is refine_ann.h; polysemous codes and `ht` are
 * polysemous_ann.h, over the handles of this header.
 *
 * Status codes and metric numbers are those of ivf_ann.h; M, nlist, k, nprobe, the ids rule and everything behind the
 * transform are those of ivfpq_ann.h.
 *
 * Semantics, fixed here once:
 *   Shape: the matrix A is fp32 [d_out][d_in], no bias.  16 <= d_out <= d_in <= 1024; d_out obeys what ivfpq_ann.h asks
 *     of d (a multiple of 16, <= 512, divisible by M); d_in need not be a multiple of anything.
 *   Preparation and inner metric:
 *     L2:            y = A x; the inner IVF-PQ index has metric L2.
 *     InnerProduct:  y = A x; the inner index has metric InnerProduct.
 *     Cosine:        x^ = x / ||x|| in fp32 by the arithmetic of ivf_ann.h's row preparation (the sum of squares in fp64,
 *                    lane l of a 64-lane wave summing components l, l + 64, ... in ascending order, then the xor tree;
 *                    norm = (float)sqrt; a zero norm counts as 1; one fp32 division per component), before any fp16
 *                    rounding; y = A x^; the inner index has metric InnerProduct -- Faiss never renormalises after a
 *                    projection, and the reference's adapter reports 1 - sim.
 *     For Cosine and InnerProduct the reported distance is 1 - sim, for L2 the distance of ivfpq_ann.h, all over y.
 *     opq_index_info reports the outer metric.
 *   Transform: y[j] = fmaf(A[j][d_in-1], x[d_in-1], ... fmaf(A[j][1], x[1], fmaf(A[j][0], x[0], 0)) ...): one fp32 FMA
 *     chain in ascending i.  A row's value depends neither on the batch it arrives in, nor on its position in the batch,
 *     nor on scheduling.  The inner index then rounds y to fp16 as it rounds any row.
 *   opq_index_load stores A as given; it does not check orthonormality.
 *   Training (the alternation of Faiss's OPQMatrix::train, made deterministic):
 *     1. X = the first min(n_train, 65536) training rows, prepared as above, fp32.
 *     2. G[j][i] = (mix64(seed + 0xD1B54A32D192ED03 (j d_in + i + 1)) >> 11) 2^-53 - 0.5 in fp64 (mix64: the 64-bit
 *        finaliser of sann_device.h); A_0 = opq_procrustes of G^T, rounded to fp32.
 *     3. niter_opq rounds (0 = 50; negative is IVF_EINVAL).  Round t:
 *        Y = A_t X by the transform above, rounded to fp16 as the inner index will store it;
 *        a product quantiser on Y itself (no residuals): M sub-quantizers of 256 codewords by squared L2, with the
 *          encoder and the mean step of ivfpq_ann.h (one all-zero centroid, every row in cell 0); round 0 picks its
 *          initial codewords by the rule of ivfpq_ann.h with this seed and runs 40 Lloyd rounds, a later round starts
 *          from the codebooks of the round before and runs 4;
 *        Y^ = the decoding of the encoding of Y, fp32;
 *        err[t] = sum ||Y - Y^||^2 / n in fp64;
 *        C = X^T Y^ ([d_in][d_out]) in fp64 on the device: every entry is summed over fixed chunks of 2048 rows in
 *          ascending row order, the chunk sums then in ascending chunk order; no floating-point atomics;
 *        A_{t+1} = opq_procrustes(C) on the host, rounded to fp32.
 *     4. The OPQ codebooks are dropped.
 *     5. The inner index is trained as ivfpq_index_train trains, on A X of all n_train rows (which stay on the device),
 *        with the caller's niter and seed.
 *     Two trainings with equal arguments give a byte-identical matrix, centroids and codebooks.  Faiss's own
 *     OPQMatrix::train (random initial rotation, its own product quantiser, LAPACK's SVD) is not vendored in the
 *     reference: parity with it is UNPINNED, exactly as the trainings of ivf_ann.h and ivfpq_ann.h are.
 *   opq_procrustes: the matrix with orthonormal rows that maximises tr(A C), i.e. (U V^T)^T of the thin singular value
 *     decomposition C = U S V^T, by a one-sided Jacobi iteration in fp64 with a fixed cyclic sweep order; left vectors of
 *     vanishing singular values are completed from the unit vectors e_0, e_1, ... in order.  Host only: it makes no
 *     device call and needs no GPU.  Deterministic.
 *
 * No function throws or aborts; every function returns a status (IVF_OK, IVF_EINVAL, ... of ivf_ann.h), the message is in
 * opq_last_error().  One call at a time per index.
 */
#ifndef OPQ_ANN_H
#define OPQ_ANN_H
#include <stdint.h>

#include "ivf_ann.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct opq_index opq_index_t;

const char *opq_last_error(void);

/* An empty index: the matrix trained on train_vectors (row-major fp32 [n_train][d_in]) as above, then the inner index
 * on the transformed rows.  n_train >= max(nlist, 256); niter and seed as in ivfpq_index_train; niter_opq >= 0. */
int opq_index_train(int32_t device, int32_t metric, int32_t d_in, int32_t d_out, int32_t nlist, int32_t M, int64_t n_train,
                    const float *train_vectors, int32_t niter, int32_t niter_opq, uint64_t seed, opq_index_t **out);
/* The same with the matrix (fp32 [d_out][d_in], kept as given), the centroids (fp32 [nlist][d_out]) and the codebooks
 * (fp32 [M][256][d_out / M]) supplied; centroids and codebooks as in ivfpq_index_load with the inner metric. */
int opq_index_load(int32_t device, int32_t metric, int32_t d_in, int32_t d_out, int32_t nlist, int32_t M, const float *A,
                   const float *centroids, const float *codebooks, opq_index_t **out);
/* As ivfpq_index_add and ivfpq_search, with rows of d_in components. */
int opq_index_add(opq_index_t *index, int64_t n, const float *vectors, const int64_t *ids);
int opq_search(opq_index_t *index, int32_t nq, const float *queries, int32_t k, int32_t nprobe, float *out_dist,
               int64_t *out_ids, int32_t *out_counts);
/* The preparation and the transform of n host rows (row-major fp32 [n][d_in]), as added rows and queries get them,
 * Cosine normalisation included: out_y is fp32 [n][d_out]. */
int opq_transform(opq_index_t *index, int64_t n, const float *x, float *out_y);

/* Rows, dimensions, the outer metric, number of cells and of sub-quantizers (any pointer may be NULL). */
int opq_index_info(const opq_index_t *index, int64_t *n, int32_t *d_in, int32_t *d_out, int32_t *metric, int32_t *nlist,
                   int32_t *M);
/* The matrix: fp32 [d_out][d_in]. */
int opq_index_get_matrix(const opq_index_t *index, float *out);
/* err[t] of the training rounds: *count of them (0 for a loaded index); out_err (double[*count]) may be NULL. */
int opq_training_errors(const opq_index_t *index, double *out_err, int32_t *count);
/* Host-clock milliseconds of the training, each phase ending in a device synchronise: the transforms, the product
 * quantiser, the decoding + error + correlation, the host's opq_procrustes, and the inner training (any may be NULL). */
int opq_training_stats(const opq_index_t *index, float *transform_ms, float *pq_ms, float *correlation_ms,
                       float *procrustes_ms, float *inner_ms);
/* The inner index's exports, as the ivfpq_* functions of these names. */
int opq_index_get_centroids(const opq_index_t *index, float *out);
int opq_index_get_codebooks(const opq_index_t *index, float *out);
int opq_index_get_codes(const opq_index_t *index, uint8_t *out);
int opq_index_list_sizes(const opq_index_t *index, int64_t *out);
int opq_index_get_assignment(const opq_index_t *index, int64_t *out_ids, int32_t *out_cells);
int opq_last_probes(const opq_index_t *index, int32_t *nq, int32_t *nprobe, int32_t *out_cells);
/* As ivfpq_last_stats, with the HIP-event milliseconds of the last search's transform kernel. */
int opq_last_stats(const opq_index_t *index, int64_t *rows_scanned, int32_t *rounds, float *coarse_ms, float *scan_ms,
                   float *select_ms, float *transform_ms);
int opq_index_destroy(opq_index_t *index);

/* The orthonormal-rows matrix A ([d_out][d_in]) that maximises tr(A C) for C ([d_in][d_out], row-major fp64).
 * 1 <= d_out <= d_in <= 1024. */
int opq_procrustes(int32_t d_in, int32_t d_out, const double *C, double *A);
/* Test seam: C = X^T Y^ by the correlation kernels of the training, for n host rows x (fp32 [n][d_in]) and y_hat
 * (fp32 [n][d_out]): out_c is double [d_in][d_out]. */
int opq_debug_correlation(int32_t device, int64_t n, int32_t d_in, int32_t d_out, const float *x, const float *y_hat,
                          double *out_c);

#ifdef __cplusplus
}
#endif
#endif
