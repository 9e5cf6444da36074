/*
 * shard_set.h -- C ABI of a set of inverted-file indexes served as one index, MI355X.
 *
 * Replaces the sharded mode of the reference's Faiss query server (all paths relative to the reference's
 * ann/src/main/scala/com/twitter/ann/):
 *   service/query_server/faiss/FaissQueryIndexServer.scala:102-112   --sharded
 *   faiss/HourlyShardedIndex.scala:66-93                             reloadShards: the newest shardedHours hourly
 *                                                                    directories as IndexShards(dimension, false, false)
 *   faiss/QueryableIndexAdapter.scala:139-178                        the search that runs over it
 * The members are indexes of ivf_ann.h, ivfpq_ann.h and opq_ann.h that the caller loaded (faiss_files.h) and goes on
 * owning; the set borrows them.  One search uploads the queries once, lets every member search them on the device, folds
 * each member's answer into a running best-k on the device and downloads one answer.
 *
 * The contract: the answer of shardset_search is byte for byte dann_compose_shards (dense_ann.h) over the members' own
 * ivf_search / ivfpq_search[_ht] / opq_search[_ht] answers at the same k, nprobe and ht: for each query the best k of all
 * members' answers by (distance ascending, id ascending), floats compared as the host compares them (-0.0 == +0.0, the tie
 * goes to the id; every distance keeps its own bits), ids as signed 64-bit integers.  Ids pass through unchanged and an id
 * that two members hold is answered twice (IndexShards with successive_ids = false).  NaN distances are outside the
 * contract; +inf is inside it.
 *
 * Out of scope: JNI methods; saving a set; members on concurrent streams; one coarse search for all members; refined
 * (refine_ann.h) members.
 *
 * Status codes are those of ivf_ann.h (IVF_OK, IVF_EINVAL, ...).  No function throws or aborts; every function returns a
 * status, the message of the last failure on this thread is in shardset_last_error().  One call at a time per set, and no
 * member may be searched elsewhere while the set searches: the set uses the members' scratch buffers.
 */
#ifndef SHARD_SET_H
#define SHARD_SET_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct shardset shardset_t;

const char *shardset_last_error(void);

/* An empty set on `device` for members of embedding dimension `dimension` (an OPQ member's d_in, an IVF-Flat or IVF-PQ
 * member's d) and of `metric` (IVF_METRIC_*). */
int shardset_create(int32_t device, int32_t dimension, int32_t metric, shardset_t **out);
/* Replaces the whole membership: kinds[i] is a FAISS_KIND_* value (faiss_files.h), handles[i] the matching ivf_index_t *,
 * ivfpq_index_t * or opq_index_t *, newest first.  n = 0 empties the set.  Kinds may be mixed.  A member of another
 * device, dimension or metric, an unknown kind or a NULL handle is IVF_EINVAL, and the membership stays what it was.
 * The handles stay the caller's: it destroys the dropped ones after this call, and the set's before or after
 * shardset_destroy. */
int shardset_set_members(shardset_t *set, int32_t n, const int32_t *kinds, void *const *handles);
/* Members, dimension, metric and the sum of the members' rows (any pointer may be NULL). */
int shardset_info(const shardset_t *set, int32_t *n_members, int32_t *dimension, int32_t *metric, int64_t *rows);
/* queries: row-major fp32 [nq][dimension].  out_dist / out_ids [nq][k], out_counts[q] = min(k, the sum of the members'
 * counts for q); slots [count, k) are zeros.  nq >= 1, 1 <= k <= 1024, 1 <= nprobe <= 1024 (clamped to each member's
 * nlist), checked before any device work.  ht <= 0: no filter; ht > 0 goes to IVF-PQ and OPQ members as
 * ivfpq_search_ht / opq_search_ht take it, and is IVF_EINVAL for a set with an IVF-Flat member.  An empty set answers
 * counts 0.  A member's failure is the call's failure, its message prefixed with the member's number. */
int shardset_search(shardset_t *set, int32_t nq, const float *queries, int32_t k, int32_t nprobe, int32_t ht,
                    float *out_dist, int64_t *out_ids, int32_t *out_counts);
/* Of the last shardset_search (any pointer may be NULL): h2d_bytes = the query upload, 4 * nq * dimension whatever the
 * number of members; d2h_result_bytes = the answer, 12 * nq * k + 4 * nq; d2h_bytes = that plus the control words the
 * member searches read back (round flags, rows counters, the flat search's group counts); HIP-event milliseconds summed
 * over the member searches and over the folds. */
int shardset_last_stats(const shardset_t *set, int64_t *h2d_bytes, int64_t *d2h_bytes, int64_t *d2h_result_bytes,
                        float *search_ms, float *fold_ms);
/* dann_compose_shards (dense_ann.h; the same arguments, host arrays in and out: ids / dist [n_shards][nq][k_in], counts
 * [n_shards][nq]) through the fold kernel on `device`, for answers that come from other GPUs.  n_shards >= 1, nq >= 0,
 * 0 <= k_in <= 1024, 1 <= k <= 1024; a count outside 0..k_in is IVF_EINVAL; every argument is checked before the first
 * device call.  Slots [count, k) of the outputs are zeros.  The runs need not be sorted. */
int shardset_compose(int32_t device, int32_t n_shards, int32_t nq, int32_t k_in, const int64_t *ids, const float *dist,
                     const int32_t *counts, int32_t k, int64_t *out_ids, float *out_dist, int32_t *out_counts);
/* NULL is allowed.  The members are not destroyed. */
int shardset_destroy(shardset_t *set);

#ifdef __cplusplus
}
#endif
#endif
