/*
 * polysemous_ann.h -- C ABI of polysemous product-quantiser codes over the IVF-PQ index of ivfpq_ann.h and the OPQ index
 * of opq_ann.h, MI355X: the renumbering of the codewords at training time, and the search that scores only the rows whose
 * code is within a Hamming distance of the query's code (Faiss's `ht`).
 *
 * What it replaces (paths relative to the reference's ann/src/main/):
 *   thrift/com/twitter/ann/common/ann_common.thrift:41-56       FaissRuntimeParam.ht, the fifth field
 *   scala/com/twitter/ann/faiss/FaissIndexer.scala:82-92        index_factory(any factory string): Faiss's index_factory
 *                                                               turns polysemous training on for every `PQ<M>` component
 *                                                               that does not end in `np`
 *   python/dataflow/faiss_index_bq_dataset.py:178-188           the default string OPQ48_240,IVF<N/20>,PQ48 is such an index
 * Not here: `ht` through refine_ann.h (the re-ranking index searches its base without a filter), the JNI methods, and the
 * three `quantizer*` fields of FaissRuntimeParam (the coarse search here is exact: the upper bound of what they tune).
 * Faiss is not vendored in the reference: parity with its permutation (PolysemousTraining, ReproduceDistancesObjective,
 * SimulatedAnnealingOptimizer), with its filter and with index_factory's polysemous default is UNPINNED, exactly as the
 * trainings of ivf_ann.h, ivfpq_ann.h and opq_ann.h are.  Speed and recall of the filter are not measured.
 *
 * Status codes, metric numbers and everything about the indexes are those of ivf_ann.h, ivfpq_ann.h and opq_ann.h.
 *
 * Semantics, fixed here once:
 *   Polysemous codes are ordinary product-quantiser codes whose codewords have been renumbered, subspace by subspace, so
 *   that the Hamming distance of two code bytes tracks the distance of their codewords.  The permutation is folded into
 *   the codebooks: an index keeps no other trace of it than a flag, and ivfpq_index_load / opq_index_load / a saved index
 *   with such codebooks is a polysemous index in all but the flag.
 *   polysemous_optimize_codebook, for one subspace of 256 codewords:
 *     Distances: D[i][j] = sum over the components c, ascending, of ((double)cb[i][c] - (double)cb[j][c])^2, in fp64.
 *     Targets:   over the 256 * 255 ordered pairs i != j, mean = sum D / count and std = sqrt(sum (D - mean)^2 / count),
 *                both sums in (i, j) order; t[i][j] = (D[i][j] - mean) / std * sqrt(2) + 4 -- 4 and sqrt(2) are the mean
 *                and the deviation of the Hamming distance of two random bytes.  std == 0 (or not finite): every target is
 *                4 and the permutation is the identity.
 *     Weights:   w[i][j] = exp(-ln 2 * t[i][j]).
 *     Cost:      cost(p) = sum over i != j, in (i, j) order, of w[i][j] * (t[i][j] - popcount(p[i] ^ p[j]))^2.
 *     Search:    simulated annealing over swaps of two labels.  draw(s, c) = mix64(seed + 0x9E3779B97F4A7C15 * (3 s + c + 1))
 *                (mix64: the 64-bit finaliser of ivfpq_ann.h's picks).  Step s = 0, 1, ...: i = draw(s, 0) mod 256;
 *                j = draw(s, 1) mod 255, plus 1 if that is >= i; u = (draw(s, 2) >> 11) * 2^-53.  The swap of the labels of
 *                codewords i and j is accepted if its delta is negative or u < T_s, as Faiss's optimizer accepts; T_0 = 0.7,
 *                T_{s+1} = T_s * 0.9^(1/500) in fp64.  The delta comes from the two affected rows in O(256):
 *                2 * sum over k != i, j, ascending, of the change of the (i, k) term plus the change of the (j, k) term.
 *                iters == 0 means 500,000 steps; negative is IVF_EINVAL.
 *     Result:    the best permutation seen by the running cost, the identity being the first candidate; out_perm[j] is the
 *                new number of old codeword j.  cost_before and cost_after are the cost formula evaluated in full on the
 *                identity and on the result; should the result not be cheaper by that evaluation, the identity is returned,
 *                so cost_after <= cost_before always holds.
 *     Determinism: the result is a function of the arguments alone.  Host only: no device call, no GPU needed.
 *   Training: ivfpq_index_train_polysemous is ivfpq_index_train followed by one polysemous_optimize_codebook per subspace m
 *     with the seed mix64(seed + 0x9E3779B97F4A7C15 * (m + 1)) and anneal_iters steps, on at most 16 host threads (the
 *     subspaces are independent: the result does not depend on the thread count); the codebooks are then renumbered on the
 *     device, new[m][perm_m[j]] = old[m][j].  The index is empty at that point: there are no codes to relabel.  Centroids
 *     are those of ivfpq_index_train byte for byte.  opq_index_train_polysemous does the same to the final inner index,
 *     after the alternation.
 *   Search: ht <= 0 disables the filter: the call is ivfpq_search / opq_search.  Otherwise, for every (query, probed cell)
 *     pair the query code is the encoding of u = fl32(q - centroid[c]) by the encoder rule of ivfpq_ann.h (squared L2 in
 *     fp32, components ascending, ties to the lower j), for all three metrics, and a row of the cell's list is scored iff
 *     the Hamming distance between its M code bytes and the pair's query code is < ht.  A row that passes gets the bits
 *     ivfpq_search gives it (the same operations in the same order); a rejected row is never a candidate, in any round of
 *     the survivor buffer.  Counts may fall short of k, down to 0.
 *
 * No function throws or aborts; every function returns a status (IVF_OK, IVF_EINVAL, ... of ivf_ann.h).  The message of
 * polysemous_optimize_codebook is in polysemous_last_error(), that of an ivfpq_* function in ivfpq_last_error(), that of
 * an opq_* function in opq_last_error().  One call at a time per index.
 */
#ifndef POLYSEMOUS_ANN_H
#define POLYSEMOUS_ANN_H
#include <stdint.h>

#include "ivf_ann.h"
#include "ivfpq_ann.h"
#include "opq_ann.h"
#ifdef __cplusplus
extern "C" {
#endif

const char *polysemous_last_error(void);

/* The renumbering of one subspace's 256 codewords (fp32 [256][dsub], 1 <= dsub <= 512, every value finite) as above. */
int polysemous_optimize_codebook(int32_t dsub, const float *codebook, int64_t iters, uint64_t seed, uint8_t *out_perm,
                                 double *cost_before, double *cost_after);

/* ivfpq_index_train, then the renumbering of every codebook (anneal_iters: 0 = 500,000 steps per subspace). */
int ivfpq_index_train_polysemous(int32_t device, int32_t metric, int32_t d, int32_t nlist, int32_t M, int64_t n_train,
                                 const float *train_vectors, int32_t niter, uint64_t seed, int64_t anneal_iters,
                                 ivfpq_index_t **out);
/* 1 for an index made by ivfpq_index_train_polysemous, 0 for any other (a loaded one included). */
int ivfpq_index_is_polysemous(const ivfpq_index_t *index, int32_t *out);
/* ivfpq_search over the rows within Hamming distance < ht of their pair's query code (ht <= 0: ivfpq_search itself). */
int ivfpq_search_ht(ivfpq_index_t *index, int32_t nq, const float *queries, int32_t k, int32_t nprobe, int32_t ht,
                    float *out_dist, int64_t *out_ids, int32_t *out_counts);
/* The query codes of the last search with ht > 0, in the order of ivfpq_last_probes: uint8 [nq][nprobe][M] (out may be
 * NULL to ask for the shape).  IVF_EINVAL before any such search. */
int ivfpq_last_query_codes(const ivfpq_index_t *index, int32_t *nq, int32_t *nprobe, uint8_t *out);
/* Of the last ivfpq_search_ht: the rows that passed the filter and were scored, out of the rows_scanned of
 * ivfpq_last_stats (the rows whose codes were read); with ht <= 0 the two are equal. */
int ivfpq_last_ht_stats(const ivfpq_index_t *index, int64_t *rows_scored);

/* The same over the OPQ index: the inner index is trained, flagged, searched and asked. */
int opq_index_train_polysemous(int32_t device, int32_t metric, int32_t d_in, int32_t d_out, int32_t nlist, int32_t M,
                               int64_t n_train, const float *train_vectors, int32_t niter, int32_t niter_opq, uint64_t seed,
                               int64_t anneal_iters, opq_index_t **out);
int opq_index_is_polysemous(const opq_index_t *index, int32_t *out);
int opq_search_ht(opq_index_t *index, int32_t nq, const float *queries, int32_t k, int32_t nprobe, int32_t ht, float *out_dist,
                  int64_t *out_ids, int32_t *out_counts);
int opq_last_query_codes(const opq_index_t *index, int32_t *nq, int32_t *nprobe, uint8_t *out);
int opq_last_ht_stats(const opq_index_t *index, int64_t *rows_scored);

#ifdef __cplusplus
}
#endif
#endif
