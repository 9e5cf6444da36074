/*
 * refine_ann.h -- C ABI of the re-ranking layer over the product-quantised indexes (Faiss's IndexRefineFlat: factory
 * suffix `,RFlat` or `,Refine(Flat)` behind `IVF<nlist>,PQ<M>` or `OPQ<M>[_<dout>],IVF<nlist>,PQ<M>`), MI355X.  The index
 * keeps the rows beside the base index, asks the base for k * k_factor candidates, recomputes their distances to the
 * stored rows and answers the best k.
 *
 * What it replaces (paths relative to the reference's ann/src/main/):
 *   scala/com/twitter/ann/faiss/FaissIndexer.scala:82-92        index_factory(any factory string) -> train -> add_with_ids
 *   thrift/com/twitter/ann/common/ann_common.thrift:49-50       "How many times more neighbours are requested from
 *                                                               underlying index by IndexRefine"
 * k_factor is a field of the Faiss index and is written with it: the offline builder sets it, no runtime parameter
 * carries it.
 * Not here: saving and loading a refined index (the container of faiss_files.h has no row section; its save functions
 * take the base handles by type), JNI methods, a refine index as the coarse quantizer (`quantizer_kfactor_rf`), by-id
 * queries over this index.
 *
 * Status codes and metric numbers are those of ivf_ann.h; the ids rule, k, nprobe and everything about the candidates are
 * those of the base (ivfpq_ann.h, opq_ann.h).
 *
 * Semantics, fixed here once:
 *   Store: the rows in the order added, prepared exactly as ivf_ann.h prepares a row: Cosine rows divided by their fp32
 *     norm (the sum of squares in fp64), then every component rounded to fp16.  Over an OPQ base these are the rows
 *     BEFORE the transform (d = d_in), as Faiss keeps them: the refined distance is a distance in the caller's space.
 *     1 <= d <= 1024 as far as the store goes (the bases ask more of d); a row occupies ceil(d / 8) * 8 halves, the
 *     padding being zero.  n < 2^31 as in the base.  Growth keeps what is there, device to device.
 *   Candidates: what the base's search answers for k' = k * k_factor and the same nprobe -- the k' nearest by the base's
 *     distance, ascending by (base distance, id) -- taken as add-order positions, not ids (ids may repeat).  Positions
 *     and counts stay on the device; the base's distances are not used.  k * k_factor <= 1024.
 *   Distance: the query is prepared as a row is.  All arithmetic is fp32, unfused (a multiply, then an add: no FMA):
 *     row and query are cut into pieces of 8 components; lane l of a 64-lane wave owns pieces l and l + 64; it starts
 *     from 0 and adds, piece by piece and within a piece in ascending component order, t * t with t = q_i - x_i (L2: the
 *     difference is taken directly, near rows do not cancel) or q_i * x_i (InnerProduct, Cosine); a lane without a piece
 *     holds 0, a padding component contributes 0.  The 64 lane sums are then added by the xor tree: for o = 32, 16, 8,
 *     4, 2, 1 every lane adds the sum of lane (l xor o).  L2: the distance is sqrtf of that; InnerProduct and Cosine:
 *     1 - that.  The order depends on d alone: not on the batch, the query's place in it, the candidate's place in its
 *     list, or scheduling.  The same (query, row) pair gives the same bits in every call.  No floating-point atomics.
 *   Answer: ascending by (distance, id); candidates equal in both come in position order.  out_counts[q] =
 *     min(k, candidates of q); slots past the count are 0 / 0, as in ivfpq_search.
 *
 * No function throws or aborts; every function returns a status (IVF_OK, IVF_EINVAL, ... of ivf_ann.h), the message is in
 * refine_last_error().  One call at a time per index.
 */
#ifndef REFINE_ANN_H
#define REFINE_ANN_H
#include <stdint.h>

#include "ivf_ann.h"
#include "ivfpq_ann.h"
#include "opq_ann.h"
#ifdef __cplusplus
extern "C" {
#endif

#define REFINE_BASE_IVFPQ 0
#define REFINE_BASE_OPQ 1
#define REFINE_MAX_K_FACTOR 1024

typedef struct refine_index refine_index_t;

const char *refine_last_error(void);

/* A refined index over a base that is trained and EMPTY (the store needs every row; a base that holds rows is
 * IVF_EINVAL).  1 <= k_factor <= 1024.  On success the handle owns the base and refine_index_destroy destroys it; on
 * failure the caller still owns it. */
int refine_index_wrap_ivfpq(ivfpq_index_t *base, int32_t k_factor, refine_index_t **out);
int refine_index_wrap_opq(opq_index_t *base, int32_t k_factor, refine_index_t **out);
/* add_with_ids: n rows (row-major fp32 [n][d], d the base's outer dimension: d_in over OPQ) go to the base and to the
 * store.  ids as in ivf_index_add.  A failed add leaves both as they were. */
int refine_index_add(refine_index_t *index, int64_t n, const float *vectors, const int64_t *ids);
/* As ivfpq_search, over the true distances of the base's k * k_factor candidates: out_dist[nq*k], out_ids[nq*k],
 * out_counts[nq].  k * k_factor > 1024 is IVF_EINVAL before any device call. */
int refine_search(refine_index_t *index, int32_t nq, const float *queries, int32_t k, int32_t nprobe, float *out_dist,
                  int64_t *out_ids, int32_t *out_counts);
/* The same with the factor of this call given; the index keeps its own. */
int refine_search_with_k_factor(refine_index_t *index, int32_t nq, const float *queries, int32_t k, int32_t nprobe,
                                int32_t k_factor, float *out_dist, int64_t *out_ids, int32_t *out_counts);
int refine_index_set_k_factor(refine_index_t *index, int32_t k_factor);

/* Rows, the outer dimension, metric, k_factor and the kind of the base, REFINE_BASE_* (any pointer may be NULL). */
int refine_index_info(const refine_index_t *index, int64_t *n, int32_t *d, int32_t *metric, int32_t *k_factor,
                      int32_t *base_kind);
/* The base, borrowed: an ivfpq_index_t * or an opq_index_t * by *base_kind, for the exports of their headers
 * (*_get_codes, *_last_probes, *_last_stats, ...).  Adding to it or destroying it is the caller's error. */
int refine_index_base(const refine_index_t *index, int32_t *base_kind, void **base);
/* The candidates of the last search: for each query the add-order positions the base handed to the re-rank, best first
 * by the base's order: int32 [nq][width] with the shape in *nq / *width (width = k * k_factor), out_counts[nq] of them
 * valid per query, -1 past the count.  out_positions NULL asks for the shape alone; out_counts may be NULL. */
int refine_last_candidates(const refine_index_t *index, int32_t *nq, int32_t *width, int32_t *out_positions,
                           int32_t *out_counts);
/* The stored halves of rows [row0, row0 + m) in the order added: uint16 [m][d] (without the padding). */
int refine_index_get_rows(const refine_index_t *index, int64_t row0, int64_t m, uint16_t *out);
/* HIP-event milliseconds of the last search: the base's search for the candidates, and the re-rank. */
int refine_last_stats(const refine_index_t *index, float *base_ms, float *rerank_ms);
/* Destroys the base too. */
int refine_index_destroy(refine_index_t *index);

#ifdef __cplusplus
}
#endif
#endif
