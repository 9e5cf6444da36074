/*
 * ann_by_id.h -- C ABI of the device-resident embedding store and of the by-id queries on the two dense indexes, MI355X.
 *
 * Replaces (all paths relative to /root/reference/ann/src/main/scala/com/twitter/ann/common/):
 *   EmbeddingProducer.scala                  trait EmbeddingProducer[T]: id -> Option[embedding]
 *   Api.scala  trait QueryableById           queryById / queryByIdWithDistance / batchQueryById / batchQueryWithDistanceById
 *   QueryableByIdImplementation.scala:15-91  EmbeddingProducer composed with a Queryable: per seed id fetch the embedding and
 *                                            query; a missing id gives nothing (:69-90); the batch form flattens the answers
 *                                            into NeighborWithDistanceWithSeed(seed, neighbor, distance) in seed order
 * The reference fetches every embedding from a key-value store and crosses a Thrift hop per seed.  Here the embeddings stay in
 * HBM beside the index: seed ids go in (8 bytes each), flattened (seed, neighbour, distance) triples come out, and no
 * embedding crosses the bus.
 *
 * The store keeps the rows as fp32, so a by-id answer is bit for bit what hnsw_search / dann_search return for the same fp32
 * row: the query preparation (fp64 sum of squares in the lane order of the plain preparation, one sqrt, fp32 divide, rounding
 * to fp16) sees the same inputs either way, and the walk / GEMM + selection kernels are the plain searches' own.
 *
 * Status codes are those of hnsw_ann.h / dense_ann.h, which agree: 0 OK, 1 EINVAL, 2 EDEVICE, 3 ELIMIT, 4 ENOMEM, 5 EINTERNAL.
 * No function throws or aborts; the message of the last failure of the calling thread is ann_by_id_last_error().
 */
#ifndef ANN_BY_ID_H
#define ANN_BY_ID_H
#include <stdint.h>

#include "dense_ann.h"
#include "hnsw_ann.h"
#ifdef __cplusplus
extern "C" {
#endif

#define ANN_BY_ID_OK 0
#define ANN_BY_ID_EINVAL 1
#define ANN_BY_ID_EDEVICE 2
#define ANN_BY_ID_ELIMIT 3
#define ANN_BY_ID_ENOMEM 4
#define ANN_BY_ID_EINTERNAL 5

typedef struct ann_store ann_store_t;

const char *ann_by_id_last_error(void);

/* The embedding store: n rows (row-major fp32 [n][d], 1 <= d <= 512, 0 <= n < 2^31 - 1) under unique int64 keys, kept on
 * `device` as fp32 beside a (key, position) table sorted by key.  A repeated key is EINVAL with a message naming it; the check
 * runs on the device (the sorted keys compared with their neighbours).  A built store is immutable -- a refresh builds a new
 * one, as the reference reloads a table -- and may serve several indexes and threads at once. */
int ann_store_build(int32_t device, int64_t n, int32_t d, const int64_t *keys, const float *vectors, ann_store_t **out);
int ann_store_info(const ann_store_t *store, int64_t *n, int32_t *d);
/* EmbeddingProducer.produceEmbedding for n keys: out_vectors [n][d] (an absent key's row is zeros), out_found [n] 1 / 0. */
int ann_store_get(const ann_store_t *store, int64_t n, const int64_t *keys, float *out_vectors, uint8_t *out_found);
int ann_store_destroy(ann_store_t *store);

/* batchQueryWithDistanceById (QueryableByIdImplementation.scala:69-90).
 *   store       the producer.  NULL: the index itself is the producer -- its keys (positions when it was created without ids)
 *               and its stored fp16 rows widened to fp32, then prepared like any query: for every metric the answer for seed s
 *               is search(*_index_get_vectors(row of s)) bit for bit.  The seed is not filtered out of its own answer.
 *   seeds       n_seeds ids, answered in request order; one given twice is answered twice
 *   out_counts  [n_seeds]: neighbours of seed i, or -1 when the store has no such key (the None branch: no triples)
 *   out_*       out_seed / out_id / out_dist [cap]: the triples of seed i before those of seed i + 1, each seed's ascending by
 *               distance -- exactly the row the plain search returns for that embedding.  *out_total of them are written and
 *               nothing beyond.
 *   cap         at least n_found * k, n_found being the seeds the store holds; less is EINVAL.  n_found is known once the
 *               seeds are resolved on the device, so this one refusal comes after the resolve and before any preparation or
 *               search; every other refusal comes before any device work.
 * Refused as the plain search refuses, with its codes: NULL arguments, k / ef out of range (hnsw: k, ef >= 1 EINVAL,
 * max(ef, k) <= 1024 ELIMIT; dann: 1 <= k <= 1024 EINVAL), n_seeds < 0 or >= 2^31 - 1, cap < 0 (n_found * k >= 2^31 - 1 is ELIMIT); also EINVAL a store of another
 * dimension or on another device than the index.  The index is left as it was.  n_seeds = 0 answers nothing.  An HNSW index
 * without a graph gives out_counts[i] = 0 for found seeds.
 * One call at a time per index, plain searches, appends and updates included (the handle's scratch is shared).
 *
 * Bus traffic of one call, as ann_by_id_last_stats reports it:
 *   host -> device   8 * n_seeds (the seed ids), plus for hnsw 4 bytes per query re-run in the second pass (the plain
 *                    search's qlist; 0 when hnsw_last_stats reports no spilled query).  The plain searches upload no other
 *                    control block, so the constant is 0.
 *   device -> host   result: 20 * out_total (the triples) + 4 * n_seeds (the counts);
 *                    control: 8 (n_found, out_total) + what the plain search reads back: hnsw 128 (its counters) + 4 * n_found
 *                    per pass (spill flags); dann 4 per re-arm round and chunk (flags), exact mode twice that. */
int hnsw_batch_query_by_id(hnsw_index_t *index, const ann_store_t *store, int32_t n_seeds, const int64_t *seeds, int32_t k,
                           int32_t ef, int64_t *out_seed, int64_t *out_id, float *out_dist, int64_t cap, int64_t *out_total,
                           int32_t *out_counts);
int dann_batch_query_by_id(dann_index_t *index, const ann_store_t *store, int32_t n_seeds, const int64_t *seeds, int32_t k,
                           int64_t *out_seed, int64_t *out_id, float *out_dist, int64_t cap, int64_t *out_total,
                           int32_t *out_counts);

/* The last by-id call on an index (exactly one of hnsw / dann is given, the other NULL; any out pointer may be NULL):
 * seeds found and absent, host -> device bytes, device -> host bytes (all, and the result part of them), and HIP-event times
 * of resolve + gather + prepare, of the search, and of the flatten (ms). */
int ann_by_id_last_stats(const hnsw_index_t *hnsw, const dann_index_t *dann, int64_t *found, int64_t *absent, int64_t *h2d_bytes,
                         int64_t *d2h_bytes, int64_t *d2h_result_bytes, float *resolve_gather_ms, float *search_ms,
                         float *flatten_ms);

#ifdef __cplusplus
}
#endif
#endif
