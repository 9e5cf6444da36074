/*
 * annoy_ann.h -- C ABI of the Annoy index (a forest of random-projection trees built on the host, a best-first walk and an
 * exact re-score on the device), MI355X.
 *
 * What it replaces (paths relative to the reference's ann/src/main/):
 *   scala/com/twitter/ann/annoy/RawAnnoyIndexBuilder.scala:53-65   append: the counter 1, 2, ... is the item's id
 *   scala/com/twitter/ann/annoy/RawAnnoyQueryIndex.scala:48-54     L2 and Cosine; InnerProduct is refused by name
 *   scala/com/twitter/ann/annoy/RawAnnoyQueryIndex.scala:124-138   nodesToExplore -> the library's search_k
 *   scala/com/twitter/ann/annoy/TypedAnnoyIndex.scala              caller ids over the counter
 *   thrift/com/twitter/ann/common/ann_common.thrift:129-133        RuntimeParams case 1, annoyParam
 * Neither Annoy library (the C++ one behind com.spotify.annoy.jni, the Java reader com.spotify.annoy.ANNIndex) is vendored
 * in the reference: parity with them is UNPINNED, like every Faiss detail.  What is stated below is the contract.
 * The reference's library also indexes a phantom all-zero item 0, because the counter starts at 1; that phantom is not
 * reproduced: the index holds the n rows given and nothing else.
 * Not here: building on the device, Annoy's file format and the index metadata file beside it, JNI methods, by-id
 * queries, membership in a ShardSet (shard_set.h).  dann_compose_shards (dense_ann.h) composes the answers of several.
 *
 * Status codes and metric numbers are those of ivf_ann.h (IVF_OK, IVF_EINVAL, IVF_EDEVICE, IVF_ELIMIT, IVF_ENOMEM,
 * IVF_EINTERNAL; IVF_METRIC_L2, IVF_METRIC_COSINE).  IVF_METRIC_INNER_PRODUCT is IVF_EINVAL, by name.
 *
 * Limits: 1 <= d <= 1024 (a row occupies ceil(d / 8) * 8 halves, the padding zero, as the store of refine_ann.h);
 *   1 <= n < 2^31; 1 <= n_trees <= 1024; n_trees * n < 2^31 (the item array is indexed by int32) and fewer than 2^31 nodes;
 *   leaf_size 2..2048, 0 meaning d + 2 (Annoy's angular node capacity); k <= 1024; search_k <= 262144 (IVF_ELIMIT).
 *
 * Semantics, fixed here once:
 *   Rows: prepared exactly as ivf_ann.h prepares a row: Cosine rows divided by their fp32 norm (the sum of squares in fp64,
 *     lane-strided partial sums met by the xor tree, as the device kernels of the siblings add them), then every component
 *     rounded to fp16.  The builder sees the rounded rows.  Rows and queries must be finite.
 *   The forest, flat: nodes int32 [n_nodes][4] = (kind, a, b, flags).  kind 0 is a split: a = left child, b = right child;
 *     kind 1 is a leaf: a = first item, b = number of items (1..leaf_size), a range of `items`.  flags bit 0
 *     (ANNOY_NODE_FALLBACK) marks a fallback split; no other bit may be set.  Splits are numbered in node order: the s-th
 *     split node owns normals[s] (d fp16 halves) and offsets[s] (fp32; 0 for Cosine).  roots int32 [n_trees];
 *     items int32 [n_trees * n]: row positions.  Tree t of a built forest occupies items [t * n, (t + 1) * n) and a
 *     contiguous run of nodes that starts at its root.
 *   The margin of a query (or row) q at a split: the dot product of the normal and q, plus, for L2, the offset, added in
 *     fp32.  The dot product is taken in the fixed fp32 order refine_ann.h states for its distance: pieces of 8 components,
 *     lane l of 64 owns pieces l and l + 64, starts from 0 and adds normal_i * q_i (an unfused multiply, then an add) piece
 *     by piece and within a piece in ascending component order; a lane without a piece holds 0, a padding component adds
 *     +0; then the xor tree over the lane sums, o = 32 down to 1.  Build and search evaluate it as the same function of the
 *     same bits, so a stored row used as a query descends to its own leaf in every tree.
 *   A split: Annoy's two-means in fp64: two distinct seed items, 200 steps that each draw an item and move the nearer
 *     running centroid (squared L2 weighted by the centroid's count; a tie moves neither), the normal is the difference of
 *     the centroids, normalised.  L2: the offset is minus the dot of the normal with the centroids' midpoint.  The normal is
 *     then rounded to fp16 and the offset recomputed from the rounded normal (fp64, rounded to fp32 once).  An item goes
 *     right where its margin is positive and left where it is negative; a margin of exactly 0 goes to the side a hash bit
 *     of (seed, tree, node serial, position) names.  A split that puts more than 0.99 of the items on one side, or whose
 *     centroids coincide, is redrawn, three times at most.  After that the node is a fallback split: flagged, normal zero,
 *     offset 0, its items alternately left and right in their current order -- identical rows still terminate.
 *     A node of at most leaf_size items is a leaf.
 *   Draws: counter-based, mix64 (the splitmix64 finaliser) chained over (seed, tree, node serial within the tree, draw
 *     number).  Tree t depends on (rows, parameters, seed, t) alone: the forest is byte-identical for every thread count,
 *     and the first T trees of a larger build are the T-tree build.
 *   The search (Annoy's get_nns_by_vector): search_k = n_trees * max(k, nodes_to_explore / n_trees) (integer division;
 *     nodes_to_explore = -1, "none", gives n_trees * k).  A priority queue of (bound, node), ordered by bound descending then
 *     node number descending, -0 counting as +0, starts with (+inf, root) of every tree.  While fewer than search_k items
 *     are collected and the queue is not empty, the maximum is popped: a leaf adds all its items to the collection (the
 *     count includes repeats across trees, as in Annoy); a split with margin m pushes (min(bound, m), right child) and
 *     (min(bound, -m), left child), min(b, v) being v where v < b and b otherwise.  The candidates are the distinct
 *     collected positions; each is scored against the stored row by refine_ann.h's distance in refine_ann.h's order
 *     (L2: sqrtf of the sum of squared differences; Cosine: 1 - dot; these are the distances of dense_ann.h -- Annoy's own
 *     angular distance sqrt(2 - 2 cos) is monotone in 1 - cos, the order is the same).
 *   Answer: the k best ascending by (distance, id); candidates equal in both come in position order.  out_counts[q] =
 *     min(k, distinct candidates of q); slots past the count are 0 / 0.  The same (query, index) gives the same bits in
 *     every call, alone or in a batch.
 *
 * No function throws or aborts; every function returns a status, the message is in annoy_last_error().  Arguments are
 * validated before any device call.  One call at a time per index; a forest is immutable and may be shared.
 */
#ifndef ANNOY_ANN_H
#define ANNOY_ANN_H
#include <stdint.h>

#include "ivf_ann.h"
#ifdef __cplusplus
extern "C" {
#endif

#define ANNOY_MAX_D 1024
#define ANNOY_MAX_TREES 1024
#define ANNOY_MAX_LEAF 2048
#define ANNOY_MAX_K 1024
#define ANNOY_MAX_SEARCH_K 262144
#define ANNOY_MAX_THREADS 16
#define ANNOY_NODE_SPLIT 0
#define ANNOY_NODE_LEAF 1
#define ANNOY_NODE_FALLBACK 1 /* flags bit 0 */

typedef struct annoy_forest annoy_forest_t;
typedef struct annoy_index annoy_index_t;

const char *annoy_last_error(void);

/* ---- the forest: host only, no device call ---- */

/* The preparation of rows and queries stated above: out is uint16 [n][d] (fp16 bits). */
int annoy_prepare_rows(int32_t metric, int32_t d, int64_t n, const float *rows_fp32, uint16_t *out);
/* Builds n_trees trees over n rows (row-major fp32 [n][d]).  threads 1..16; 0 means min(16, n_trees); the threads split
 * the trees. */
int annoy_forest_build(int32_t metric, int32_t d, int64_t n, const float *rows_fp32, int32_t n_trees, int32_t leaf_size,
                       uint64_t seed, int32_t threads, annoy_forest_t **out);
/* The flat form from the caller, validated before anything keeps it: every child index in range; every tree a tree (each
 * node reached exactly once, from exactly one root); every position 0..n-1 in exactly one leaf of every tree; leaves of
 * 1..leaf_size items; kinds and flags known; offsets and normals finite.  Anything else is IVF_EINVAL. */
int annoy_forest_load(int32_t metric, int32_t d, int64_t n, int32_t n_trees, int32_t leaf_size, int64_t n_nodes,
                      const int32_t *nodes, int64_t n_splits, const uint16_t *normals, const float *offsets,
                      const int32_t *roots, int64_t n_items, const int32_t *items, annoy_forest_t **out);
/* Any pointer may be NULL.  leaf_size is the effective one (never 0). */
int annoy_forest_info(const annoy_forest_t *forest, int32_t *metric, int32_t *d, int64_t *n, int32_t *n_trees,
                      int32_t *leaf_size, int64_t *n_nodes, int64_t *n_splits, int64_t *n_items);
int annoy_forest_get_nodes(const annoy_forest_t *forest, int32_t *out);    /* [n_nodes][4] */
int annoy_forest_get_normals(const annoy_forest_t *forest, uint16_t *out); /* [n_splits][d] */
int annoy_forest_get_offsets(const annoy_forest_t *forest, float *out);    /* [n_splits] */
int annoy_forest_get_roots(const annoy_forest_t *forest, int32_t *out);    /* [n_trees] */
int annoy_forest_get_items(const annoy_forest_t *forest, int32_t *out);    /* [n_items] */
int annoy_forest_destroy(annoy_forest_t *forest);

/* ---- the index ---- */

/* The index over a forest and the rows it was built from (fp32 [n][d]; prepared again here, to the same bits).  The forest
 * is copied: the caller keeps and destroys its own.  ids NULL: 1..n, the counter of RawAnnoyIndexBuilder.  The index is
 * immutable: toQueryable ends the builder. */
int annoy_index_from_forest(int32_t device, const annoy_forest_t *forest, const float *rows_fp32, const int64_t *ids,
                            annoy_index_t **out);
/* annoy_forest_build, then annoy_index_from_forest. */
int annoy_index_build(int32_t device, int32_t metric, int32_t d, int64_t n, const float *rows_fp32, const int64_t *ids,
                      int32_t n_trees, int32_t leaf_size, uint64_t seed, int32_t threads, annoy_index_t **out);
/* out_dist[nq*k], out_ids[nq*k], out_counts[nq].  nodes_to_explore -1 = none, otherwise >= 0.  k > 1024 or a search_k above
 * 262144 is IVF_ELIMIT before any device call. */
int annoy_search(annoy_index_t *index, int32_t nq, const float *queries, int32_t k, int32_t nodes_to_explore, float *out_dist,
                 int64_t *out_ids, int32_t *out_counts);
int annoy_index_info(const annoy_index_t *index, int64_t *n, int32_t *d, int32_t *metric, int32_t *n_trees,
                     int32_t *leaf_size, int64_t *n_nodes);
/* The stored halves of rows [row0, row0 + m): uint16 [m][d] (without the padding). */
int annoy_index_get_rows(const annoy_index_t *index, int64_t row0, int64_t m, uint16_t *out);
/* The index's forest, borrowed: it lives as long as the index; destroying it is the caller's error. */
int annoy_index_forest(const annoy_index_t *index, const annoy_forest_t **out);
/* The candidates of the last search: the distinct positions per query, ascending: int32 [nq][width] with the shape in
 * *nq / *width, out_counts[nq] of them valid per query, -1 past the count.  out_positions NULL asks for the shape alone.
 * A batch whose candidate lists would take more than 256 MiB does not keep them: IVF_ELIMIT. */
int annoy_last_candidates(const annoy_index_t *index, int32_t *nq, int32_t *width, int32_t *out_positions, int32_t *out_counts);
/* Of the last search: per query the pops and the items collected (repeats included), int32 [nq] each (NULL: not wanted);
 * the queries re-run with a larger queue, the slices the batch ran in, and HIP-event milliseconds of the walk, the scoring
 * and the selection, summed over the slices. */
int annoy_last_stats(const annoy_index_t *index, int32_t *out_pops, int32_t *out_collected, int32_t *rerun, int32_t *slices,
                     float *walk_ms, float *score_ms, float *select_ms);
/* For tests: the queue capacity of the first launch (a query that outgrows it is re-run with room for every node, so the
 * answer never changes) and the scratch budget of one launch in bytes (a batch that needs more runs in slices of
 * queries).  0 means the default. */
int annoy_debug_set_limits(annoy_index_t *index, int64_t first_queue_capacity, int64_t scratch_budget_bytes);
int annoy_index_destroy(annoy_index_t *index);

#ifdef __cplusplus
}
#endif
#endif
