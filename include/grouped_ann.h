/*
 * grouped_ann.h -- C ABI of the grouped index: every row carries a group number, a query names the group whose rows
 * answer it, MI355X.
 *
 * Replaces the grouped mode of the reference's query servers (all paths relative to the reference's ann/src/main/):
 *   scala/com/twitter/ann/dataflow/offline/ANNIndexBuilderBeamJob.scala:192-216   GroupedEmbeddingData.groupId,
 *                                                                                 groupBy(_.getKey): one index per key
 *   scala/com/twitter/ann/common/Api.scala:54-85                                  QueryableGrouped: query(..., key)
 *   scala/com/twitter/ann/service/query_server/common/RefreshableQueryable.scala:47-55,131-177
 *                                                                                 Map[Option[String], Queryable]; a key
 *                                                                                 that is not in the map answers List()
 *   scala/com/twitter/ann/service/query_server/common/QueryIndexThriftController.scala:42-57   query.key
 *   thrift/com/twitter/ann/common/ann_common.thrift:16-19                         enum DistanceMetric
 * The reference holds one HNSW or Faiss index per key.  Here all groups are one index: the IVF-Flat list layout of
 * ivf_ann.h with cell = group (every group starts on a 32-row block, rows in (group, id) order), and one search serves a
 * batch of queries on any mix of groups.  The search is exact within the group: the upper bound of what the per-group
 * approximate index finds.  The key <-> group-number table is the caller's (the Python mirror keeps it).
 *
 * Arithmetic: as in dense_ann.h and ivf_ann.h.  Rows and queries are rounded to fp16 (Cosine: L2-normalised first, the
 * index then behaves as InnerProduct), products accumulate in fp32 on the matrix cores.  Distances are those of
 * dense_ann.h (L2 = ||q - x||, Cosine = 1 - cos, InnerProduct = 1 - <q, x>).
 *
 * Semantics, fixed here once:
 *   The index is immutable: the reference swaps the whole mapping on refresh (RefreshableQueryable.innerLoad), so there
 *     is no append.
 *   A query's answer is a function of its group's rows, the query and k alone: its bytes do not depend on the other
 *     queries of the batch, on the other groups of the index or on scheduling.
 *   A query group < 0 or >= n_groups is the reference's "key not in the mapping": count 0, not an error.  An empty group
 *     answers 0 too.
 *
 * Out of scope: saving and loading a grouped index; reading the reference's per-group directories; JNI methods;
 * approximate per-group indexes (HNSW or IVF inside a group); appending.
 *
 * Status codes carry the numbers of ivf_ann.h.  No function throws or aborts; every function returns a status, the
 * message of the last failure is in gann_last_error().  One call at a time per index.
 */
#ifndef GROUPED_ANN_H
#define GROUPED_ANN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GANN_OK 0
#define GANN_EINVAL 1
#define GANN_EDEVICE 2
#define GANN_ELIMIT 3
#define GANN_ENOMEM 4    /* host allocation failed */
#define GANN_EINTERNAL 5 /* an unexpected C++ exception was caught at the ABI; the message says which */

/* ann_common.thrift:16-19 */
#define GANN_METRIC_L2 0
#define GANN_METRIC_COSINE 1
#define GANN_METRIC_INNER_PRODUCT 2

typedef struct gann_index gann_index_t;

const char *gann_last_error(void);

/* vectors: row-major fp32 [n][d]; ids: int64 [n], or NULL (ids = positions); groups: int32 [n], the group of every row.
 * d a multiple of 16 and <= 512; 1 <= n_groups <= 1048576; 0 <= n < 2^31 - 64.  A group number outside [0, n_groups) is
 * GANN_EINVAL with a message naming the first such row, found on the host before any device call.  A group may be
 * empty. */
int gann_index_build(int32_t device, int32_t metric, int32_t d, int32_t n_groups, int64_t n, const float *vectors,
                     const int64_t *ids, const int32_t *groups, gann_index_t **out);
/* nq queries (row-major fp32 [nq][d]) with their groups (int32 [nq]): for each, the exact k nearest rows of its group and
 * no other row, ascending by (distance, id): out_dist[nq*k], out_ids[nq*k], out_counts[nq] = min(k, size of the group),
 * 0 for a group outside [0, n_groups).  1 <= k <= 1024, nq any positive int32.  More than 8192 rows of the group tying
 * at a query's k-th distance is GANN_ELIMIT; the index stays usable. */
int gann_search(gann_index_t *index, int32_t nq, const float *queries, const int32_t *query_groups, int32_t k,
                float *out_dist, int64_t *out_ids, int32_t *out_counts);

/* Rows, dimension, metric and number of groups (any pointer may be NULL). */
int gann_index_info(const gann_index_t *index, int64_t *n, int32_t *d, int32_t *metric, int32_t *n_groups);
/* Rows per group: int64 [n_groups]. */
int gann_index_group_sizes(const gann_index_t *index, int64_t *out);
/* Of the last gann_search (any pointer may be NULL): tiles = the groups of <= 32 queries on one key; work_items = the
 * (tile, segment) workgroups launched in round 0; rounds = 1, plus one per fallback round in which some query held more
 * candidates than its survivor buffer (8192) and was scanned again above a threshold; rows_scanned = the sum over
 * queries of their group's size; segment_rows = the rows of a list segment; HIP-event milliseconds of the sort /
 * work-list step, the scan rounds and the selection. */
int gann_last_stats(const gann_index_t *index, int64_t *tiles, int64_t *work_items, int32_t *rounds, int64_t *rows_scanned,
                    int32_t *segment_rows, float *worklist_ms, float *scan_ms, float *select_ms);
int gann_index_destroy(gann_index_t *index);

#ifdef __cplusplus
}
#endif
#endif
