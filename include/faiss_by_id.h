/*
 * faiss_by_id.h -- C ABI of the by-id queries on the inverted-file family and on shard sets, MI355X.
 *
 * Replaces, for the indexes of ivf_ann.h, ivfsq_ann.h, ivfpq_ann.h / polysemous_ann.h, opq_ann.h and shard_set.h, what
 * ann_by_id.h replaces for the two dense indexes (paths relative to the reference's ann/src/main/scala/com/twitter/ann/common/):
 *   Api.scala  trait QueryableById           queryById / queryByIdWithDistance / batchQueryById / batchQueryWithDistanceById
 *   QueryableByIdImplementation.scala:15-91  EmbeddingProducer composed with a Queryable; a missing id gives nothing (:69-90);
 *                                            the batch form flattens into NeighborWithDistanceWithSeed in seed order
 * The producer is the device-resident store of ann_by_id.h (ann_store_build): seed ids go in (8 bytes each), flattened
 * (seed, neighbour, distance) triples come out, and no embedding crosses the bus.
 *
 * One call is: resolve the seeds in the store's key table -> compact the found seeds in request order -> read their rows
 * through the position list straight into the index's own query preparation (no fp32 copy of the gathered rows; OPQ: the
 * transform's tile load goes through the list; a shard set: one plain fp32 row copy into the set's query buffer, which every
 * member then prepares for itself) -> the index's own search on the device -> flatten.
 *
 * The contract: for every index kind, metric, nprobe and ht, the triples of a found seed s are byte for byte row s of the
 * plain search (ivf_search, ivfsq_search, ivfpq_search_ht, opq_search_ht, shardset_search) over ann_store_get(store, s):
 * ids, distance bits and counts.  The preparation reads the same fp32 values and runs the plain preparation's arithmetic
 * (fp64 sum of squares, lane l summing elements l, l + 64, ... in that order; one sqrt; fp32 divide; rounding to fp16), and
 * everything after it is the plain search's own code.
 *
 * The store keeps rows of 1 <= d <= 512, which caps an OPQ index's d_in on this path (opq_ann.h itself allows 1024).
 *
 * Out of scope: the index as its own producer (it keeps codes or fp16 rows in list order, not the fp32 rows: that would be a
 * reconstruction); refined (refine_ann.h, `,RFlat`) indexes; Annoy; the EditDistance index; grouped indexes; JNI methods; a
 * store wider than 512; any change to the nlist, k or nprobe limits.
 *
 * Status codes are those of ann_by_id.h / ivf_ann.h, which agree: 0 OK, 1 EINVAL, 2 EDEVICE, 3 ELIMIT, 4 ENOMEM,
 * 5 EINTERNAL.  No function throws or aborts; the message of the last failure of the calling thread is
 * ivf_by_id_last_error().
 *
 * On the names: the library's exported `faiss_*` symbols are exactly those of faiss_files.h and its `shardset_*` symbols
 * exactly those of shard_set.h (tests/test_faiss_files_cpu.py and tests/test_shard_set_cpu.py hold the library to that), so
 * the two functions that serve every kind here are ivf_by_id_*, and the set's entry point is shard_set_batch_query_by_id.
 */
#ifndef FAISS_BY_ID_H
#define FAISS_BY_ID_H
#include <stdint.h>

#include "ann_by_id.h"
#include "ivf_ann.h"
#include "ivfpq_ann.h"
#include "ivfsq_ann.h"
#include "opq_ann.h"
#include "shard_set.h"
#ifdef __cplusplus
extern "C" {
#endif

/* what ivf_by_id_last_stats is asked about: the first three are the FAISS_KIND_* numbers of faiss_files.h */
#define FAISS_BY_ID_IVF_FLAT 1
#define FAISS_BY_ID_IVF_PQ 2
#define FAISS_BY_ID_OPQ_IVF_PQ 3
#define FAISS_BY_ID_IVF_SQ8 4
#define FAISS_BY_ID_SHARD_SET 5

const char *ivf_by_id_last_error(void);

/* batchQueryWithDistanceById (QueryableByIdImplementation.scala:69-90) on an index of the family.
 *   store       the producer; its d is the index's (an OPQ index's d_in, a set's dimension) and its device the index's.
 *               NULL is EINVAL: these indexes keep no fp32 rows of their own to be their own producer.
 *   seeds       n_seeds ids, answered in request order; one given twice is answered twice
 *   nprobe      as the plain search takes it (clamped to nlist); ht (ivfpq / opq / shardset): <= 0 no filter, as
 *               ivfpq_search_ht; > 0 on a set with an IVF-Flat member is EINVAL, as shardset_search
 *   out_counts  [n_seeds]: neighbours of seed i, or -1 when the store has no such key (the None branch: no triples).  The
 *               count can be less than k: the probed lists, or a set's members, may hold fewer rows
 *   out_*       out_seed / out_id / out_dist [cap]: the triples of seed i before those of seed i + 1, each seed's ascending by
 *               distance -- exactly the row the plain search returns for that embedding, the seed itself included when the
 *               index holds it.  *out_total of them are written and nothing beyond.
 *   cap         at least n_found * k, n_found being the seeds the store holds; less is EINVAL.  n_found is known once the
 *               seeds are resolved on the device, so this refusal (and ELIMIT for n_found * k >= 2^31 - 1) comes after the
 *               resolve and before any preparation or search; every other refusal comes before any device work.
 * EINVAL before any device work, the index left as it was: NULL arguments (out_seed / out_id / out_dist may be NULL when cap
 * is 0, seeds and out_counts when n_seeds is 0), k or nprobe outside 1..1024, n_seeds < 0 or >= 2^31 - 1, cap < 0, a NULL
 * store, a store of another dimension or on another device than the index.  n_seeds = 0 answers nothing.  When every seed is
 * absent nothing is prepared and nothing is searched.  A failure of the plain search (IVF_ELIMIT: the tie mass at the k-th
 * distance of a query is above the survivor cap) is returned as it is, with the search's message.
 * One call at a time per index or set, plain searches and adds included (the handle's scratch is shared).  An index with an
 * HNSW coarse quantizer attached (ivf_hnsw_quantizer.h) is served through the same path: a probe its walk misses is
 * exported as -1 by *_last_probes, as after a plain search. */
int ivf_batch_query_by_id(ivf_index_t *index, const ann_store_t *store, int32_t n_seeds, const int64_t *seeds, int32_t k,
                          int32_t nprobe, int64_t *out_seed, int64_t *out_id, float *out_dist, int64_t cap, int64_t *out_total,
                          int32_t *out_counts);
int ivfsq_batch_query_by_id(ivfsq_index_t *index, const ann_store_t *store, int32_t n_seeds, const int64_t *seeds, int32_t k,
                            int32_t nprobe, int64_t *out_seed, int64_t *out_id, float *out_dist, int64_t cap, int64_t *out_total,
                            int32_t *out_counts);
int ivfpq_batch_query_by_id(ivfpq_index_t *index, const ann_store_t *store, int32_t n_seeds, const int64_t *seeds, int32_t k,
                            int32_t nprobe, int32_t ht, int64_t *out_seed, int64_t *out_id, float *out_dist, int64_t cap,
                            int64_t *out_total, int32_t *out_counts);
int opq_batch_query_by_id(opq_index_t *index, const ann_store_t *store, int32_t n_seeds, const int64_t *seeds, int32_t k,
                          int32_t nprobe, int32_t ht, int64_t *out_seed, int64_t *out_id, float *out_dist, int64_t cap,
                          int64_t *out_total, int32_t *out_counts);
int shard_set_batch_query_by_id(shardset_t *set, const ann_store_t *store, int32_t n_seeds, const int64_t *seeds, int32_t k,
                               int32_t nprobe, int32_t ht, int64_t *out_seed, int64_t *out_id, float *out_dist, int64_t cap,
                               int64_t *out_total, int32_t *out_counts);

/* The last by-id call on `handle`, an index or set of the kind FAISS_BY_ID_* names (any out pointer may be NULL):
 *   found, absent       found + absent = n_seeds
 *   h2d_bytes           8 * n_seeds (the seed ids) plus what the search uploads as control: 0 with the exhaustive coarse
 *                       quantizer; with an HNSW quantizer 4 bytes per query its walk re-runs in a second pass
 *   d2h_result_bytes    20 * out_total (the triples) + 4 * n_seeds (the counts)
 *   d2h_bytes           that plus 8 (n_found, out_total) plus the control words the search reads back (round flags, rows
 *                       counters, the flat scan's group counts; for a set, of every member)
 *   resolve_gather_ms   HIP-event time from the seed upload to the compacted position list
 *   search_ms           of the search, the fused gather + preparation included (0 when every seed is absent)
 *   flatten_ms          of the count scan and the flatten kernel */
int ivf_by_id_last_stats(int32_t kind_or_set, const void *handle, int64_t *found, int64_t *absent, int64_t *h2d_bytes,
                           int64_t *d2h_bytes, int64_t *d2h_result_bytes, float *resolve_gather_ms, float *search_ms,
                           float *flatten_ms);

#ifdef __cplusplus
}
#endif
#endif
