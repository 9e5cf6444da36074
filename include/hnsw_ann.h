/*
 * hnsw_ann.h -- C ABI of the HNSW graph search (ann/hnsw), MI355X.
 *
 * Replaces the query side of the reference's Java HNSW (all paths relative to
 * /root/reference/ann/src/main/):
 *   java/com/twitter/ann/hnsw/HnswIndex.java:538-553    searchKnn(query, numOfNeighbours, ef)
 *   java/com/twitter/ann/hnsw/HnswIndex.java:447-475    bestEntryPointUntilLayer (greedy descent)
 *   java/com/twitter/ann/hnsw/HnswIndex.java:571-623    searchLayerForCandidates (beam search, layer 0)
 *   java/com/twitter/ann/hnsw/DistancedItemQueue.java   min / max queues = java.util.PriorityQueue ordered by
 *                                                       Float.compare on the distance (:37-43)
 *   scala/com/twitter/ann/hnsw/Hnsw.scala:95-147        queryWithDistance: ef from HnswParams, Cosine =
 *                                                       normalised vectors + InnerProduct (:139-155)
 *   scala/com/twitter/ann/hnsw/DistanceFunctionGenerator.scala:12-30
 * The graph is data: `Map<HnswNode(level, item), ImmutableList<item>>` + HnswMeta(maxLevel, entryPoint)
 * (HnswIndex.java:56-72), what HnswIndexIOUtil reads from an index directory.  hnsw_index_build takes
 * exactly that, as flat arrays.  hnsw_index_build_insert builds a graph with the reference's insertion
 * algorithm (HnswIndex.java:137-200,384-440,479-526) on the host; the reference builds offline (SURVEY 8
 * row D4) and any graph it wrote can be loaded instead.
 *
 * Search results are a function of (graph, float distances): the walk reproduces the reference step by
 * step, including java.util.PriorityQueue's sift order, so equal distances are handled as the JVM would.
 * Distances: vectors and queries rounded to fp16, products and sums in fp32 in a fixed order (8 strided
 * partial sums of 8-element chunks, then a pairwise tree) that oracle/hnsw_oracle.c repeats bit for bit.
 * The reference's own fp32 arithmetic (EmbeddingMath, un-vendored) is not pinned by any fixture: parity
 * with the JVM is "unpinned" in the float distances, exact in the walk given the distances.
 */
#ifndef HNSW_ANN_H
#define HNSW_ANN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define HNSW_OK 0
#define HNSW_EINVAL 1
#define HNSW_EDEVICE 2
#define HNSW_ELIMIT 3
#define HNSW_ENOMEM 4    /* host allocation failed */
#define HNSW_EINTERNAL 5 /* an unexpected C++ exception was caught at the ABI; the message says which */

/* ann_common.thrift:16-19 */
#define HNSW_METRIC_L2 0
#define HNSW_METRIC_COSINE 1
#define HNSW_METRIC_INNER_PRODUCT 2

typedef struct hnsw_index hnsw_index_t;

const char *hnsw_last_error(void);

/* Load a graph.  Items are positions 0..n-1 of `vectors` (row-major fp32 [n][d], d <= 512); `ids` (or NULL =
 * position) are what searches return.  Graph entry e is HnswNode(entry_level[e], entry_item[e]) with
 * neighbours entry_neighbours[entry_offsets[e] .. entry_offsets[e+1]) in list order.  max_m bounds the
 * lists: 2*max_m at level 0, max_m above (HnswIndex.java:117).  entry_point < 0 = empty index. */
int hnsw_index_build(int32_t device, int32_t metric, int64_t n, int32_t d, const float *vectors, const int64_t *ids,
                     int32_t max_m, int64_t entry_point, int32_t max_level, int64_t n_entries, const int32_t *entry_level,
                     const int64_t *entry_item, const int64_t *entry_offsets, const int64_t *entry_neighbours,
                     hnsw_index_t **out);

/* Build the graph with the reference's insertion algorithm (HnswIndex.insert), then load it.
 * Level draw: (int)(-ln(U) / ln(max_m)) with U from a 64-bit mixer of (seed, item) (HnswIndex.java:118,369-371).
 * n_threads = 1 inserts items 0..n-1 in order: deterministic.  With more host threads items are inserted
 * concurrently under per-item locks, as the reference's writers do (HnswIndex.java:150-200): the graph then
 * depends on the interleaving (and, as the reference notes at :376-380, may miss a few links). */
int hnsw_index_build_insert(int32_t device, int32_t metric, int64_t n, int32_t d, const float *vectors, const int64_t *ids,
                            int32_t max_m, int32_t ef_construction, uint64_t seed, int32_t n_threads, hnsw_index_t **out);

/* The graph back as flat arrays (two calls: sizes, then contents) and the stored (fp16-rounded) vectors. */
/* The same, with every item's level given by the caller instead of drawn (the reference draws it from a thread-local
 * Random, HnswIndex.java:369-371): a deterministic rebuild, and the form the oracle's restatement of insert is compared
 * with (tests/test_hnsw_build_gpu.py).  levels[i] in 0..60. */
int hnsw_index_build_insert_levels(int32_t device, int32_t metric, int64_t n, int32_t d, const float *vectors,
                                   const int64_t *ids, int32_t max_m, int32_t ef_construction, const int32_t *levels,
                                   int32_t n_threads, hnsw_index_t **out);
/* Build on the device, every step of it, and deterministically: two builds of one input give one graph.  The reference's
 * multi-writer insertion (HnswIndex.java:150-200; "when using concurrent writers we can miss connections", :376-380) with the
 * interleaving fixed:
 *   order   items by (level descending, position ascending); the first is the entry point and carries maxLevel
 *   rounds  the next min(batch, max(1, linked / 8)) items of the order are inserted against ONE snapshot of the graph
 *   A       per item, wireConnectionForAllLayers (:137-148): bestEntryPointUntilLayer, then per layer
 *           searchLayerForCandidates(efConstruction), selectNearestNeighboursByHeuristic(maxM), the item's own list,
 *           neighbours.get(0) as the next layer's entry; back links are recorded as (layer, neighbour, order index)
 *   B       per (layer, node), all its additions of the round in order-index order: appended while the list has room
 *           (:414-417), else one re-selection by the heuristic over old list ++ additions sorted ascending by
 *           (Float.compare distance, position) (:419-427 does that per addition)
 * Bounds the reference does not have, counted in hnsw_index_build_stats: a walk's candidate queue holds 1024 entries (when
 * full, entries beyond the current bound -- never expanded, :589-591 -- are dropped and the heap rebuilt in array order); a
 * re-selection sees the first 1024 of old list ++ additions.  oracle/hnsw_oracle.c restates exactly this
 * (oracle_hnsw_build_batched); tests/test_hnsw_gpu_build_gpu.py compares the graphs entry for entry.
 * ef_construction <= 256; batch = items per round (0 = 4096).  _levels: every item's level given (0..60) instead of drawn. */
int hnsw_index_build_insert_gpu(int32_t device, int32_t metric, int64_t n, int32_t d, const float *vectors, const int64_t *ids,
                                int32_t max_m, int32_t ef_construction, uint64_t seed, int32_t batch, hnsw_index_t **out);
int hnsw_index_build_insert_gpu_levels(int32_t device, int32_t metric, int64_t n, int32_t d, const float *vectors, const int64_t *ids,
                                       int32_t max_m, int32_t ef_construction, const int32_t *levels, int32_t batch, hnsw_index_t **out);
/* Hnsw.append / HnswIndex.insert (Hnsw.scala:86-114, HnswIndex.java:153-200) for n more rows, on the device, with the rounds
 * of the device builder above continued on the live graph.  Works on an index from any constructor (a loaded graph, the host
 * builder, the device builder).
 *   rows    the new rows take positions n_old .. n_old + n - 1; vectors is row-major fp32 [n][d] with the index's d, prepared
 *           as at build time (fp16 rows, normalised for Cosine)
 *   keys    an index created with ids needs ids (n keys); one created without needs ids = NULL, its keys being positions.  A
 *           key already in the index or repeated among the n is IllegalDuplicateInsertException: HNSW_EINVAL, message naming it.
 *           The check runs on the device against a sorted copy of the index's keys, kept on the handle from the first append
 *   levels  _levels: given, each in 0..60.  Otherwise drawn with the builder's formula at the row's GLOBAL position, so that
 *           build(X0, seed) then append(X1, seed) draws the levels of build(X0 ++ X1, seed)
 *   order   the new rows by (level descending, position ascending)
 *   rounds  the builder's schedule continued: min(batch, max(1, linked / 8), remaining) rows per round, linked = n_old at the
 *           start; batch 0 = 4096.  Each round is phases A and B of the builder against one snapshot
 *   entry   a new row above the graph's maxLevel is wired on the layers up to the old maxLevel from the old entry point, within
 *           its round's snapshot; after that round it is the entry point and maxLevel is its level (HnswIndex.java:163-198 with
 *           the round as the unit of interleaving; of several such rows in one round the first in order wins).  Later rounds
 *           walk from it.  Appending to an empty index makes the first new row in order the entry point, as a build does
 * So append(build_gpu(X0), X1) with every new row at level 0 and n_old on a round boundary of the schedule is the device
 * build of X0 ++ X1 (tests/test_hnsw_append_gpu.py holds it against oracle_hnsw_build_batched).
 * Refused with HNSW_EINVAL before anything changes: a duplicate key, ids present or absent contrary to the index, a level
 * outside 0..60, ef_construction outside 1..256, batch outside 0..2^20, n_old + n >= 2^31 - 1.  A device error part-way
 * leaves the index unusable: every later call on it fails with HNSW_EDEVICE.
 * Room: the buffers grow by 1.5x at least, device to device (exactly to the capacity after hnsw_index_reserve).  An append
 * touches no host copy of the lists: the first export (hnsw_index_graph_size, hnsw_index_graph) or save after it reads them from
 * the device, and that read is kept until the next append or update.
 * One call at a time per index, appends and searches alike (the handle's scratch is shared), as for hnsw_search.
 * hnsw_index_build_stats reports the last append. */
int hnsw_index_append(hnsw_index_t *index, int64_t n, const float *vectors, const int64_t *ids, int32_t ef_construction,
                      uint64_t seed, int32_t batch);
int hnsw_index_append_levels(hnsw_index_t *index, int64_t n, const float *vectors, const int64_t *ids, int32_t ef_construction,
                             const int32_t *levels, int32_t batch);
/* Hnsw.update (Hnsw.scala:161-181, SerializableHnsw.scala:191-195; trait Updatable, Api.scala:147-150) for n rows, on the device:
 * the embedding of a key already in the index is overwritten and the key re-inserted (HnswIndex.reInsert, HnswIndex.java:220-329);
 * a key not in the index is inserted.
 *   keys     ids is required.  On an index created with ids they are keys: present keys are updated, then the absent ones are
 *            appended in request order by hnsw_index_append (same ef_construction, seed and batch; levels drawn at their global
 *            positions), so update(P ++ A) is update(P) then append(A); *out_appended (may be NULL) is their number.  On an index
 *            created without ids they are positions, each < n: there is no upsert.  The key -> position table lives on the device
 *            (built at the first update, rebuilt after an append)
 *   rows     prepared as at build time (fp16, normalised for Cosine, Hnsw.scala:149-155)
 *   rounds   the present rows in request order, `batch` per round (0 = 4096); each round, in this order:
 *     1 vectors  the round's rows are written
 *     2 relink   (:251-324) for each item u and each layer l = 0 .. top(u) with N_l(u) non-empty, where top(u) is the highest layer
 *                <= maxLevel holding HnswNode(l, u) (:244-250; the existence the export shows: a key loaded or wired, or a non-empty
 *                list).  setCand = u, then each e of N_l(u) in list order followed by N_l(e) in list order, first occurrence kept
 *                (the reference's HashSet order is unspecified: insertion order is this library's choice).  For every v of N_l(u)
 *                other than u (updateNeighborProbability = 1, :125,271) a proposal for v's list: setCand \ {v} offered in that
 *                order to a max queue of min(efC, |set|) entries with the replacement rule of :292-309, then
 *                selectNearestNeighboursByHeuristic with maxM0 on layer 0 and maxM above (:311-314).  All proposals read the graph
 *                as the round found it; of several proposals for one (l, v) the latest item in request order wins (a later
 *                reInsert overwrites an earlier one), the others are counted as superseded.  setCand is enumerated without a cap
 *                (at most 1 + 2maxM + 4maxM^2 entries)
 *     3 wire     (:328, wireConnectionForAllLayers(..., isUpdate = true)) the builder's phase A with the item's level = top(u) and
 *                the index's entry point and maxLevel, which an update never changes.  The walk puts u in the candidate queue but
 *                not the result queue (:607-609); when u is the entry point the walk starts at u and the heuristic drops it
 *                (:488-491, :505-507).  The items' new lists (maxM entries on every layer, :392) are committed after every walk of
 *                the round has ended.  A layer whose heuristic keeps nobody keeps u's old list and the walk continues from u (the
 *                reference throws at neighbours.get(0), :439): counted as lists_kept
 *     4 links    the builder's phase B over the round's items; an addition of u to a list that already holds u -- judged on the
 *                graph after the commits of steps 2 and 3 -- is dropped and counted (:405-412)
 *            A row without HnswNode(0, u), or any row of an index whose graph is empty, has its vector written and nothing else
 *            (the reference's checkState fails there, :231-240).
 * With batch = 1 this is the reference's single-writer sequence of reInsert calls, up to the builder's candidate-queue bound
 * (BUILD_CCAP, see hnsw_index_build_insert_gpu) and, in a full re-selection of step 4, ties in distance broken by position
 * instead of heap order.  tests/hnsw_update_ref.c restates both the rounds and the unbatched reInsert.
 * Refused with HNSW_EINVAL before anything changes: a key repeated in the call, a position out of range, ef_construction outside
 * 1..256, batch outside 0..2^20, NULL vectors or ids, n_old + (absent keys) >= 2^31 - 1, more than 2^27 relink proposal slots in
 * one round (batch * layers * 2maxM; not reachable with batch <= 2^20 at usual level counts).  A device error part-way leaves the
 * index unusable (as an append does).  If the append of the absent keys fails after the rounds (device memory for its growth,
 * a device error), the present keys stay updated, the absent ones are not added, and the message says so; the index is then as
 * after update(P) (or unusable, for a device error part-way through the append).
 * The next export reads the lists from the device again.  One call at a time per index, as for appends and searches. */
int hnsw_index_update(hnsw_index_t *index, int64_t n, const float *vectors, const int64_t *ids, int32_t ef_construction,
                      uint64_t seed, int32_t batch, int64_t *out_appended);
/* Counters of the last hnsw_index_update (any pointer may be NULL): rounds, relink proposals, proposals superseded by a later item
 * of their round, back-link additions dropped because the list held the item already, distance evaluations of steps 2-4, and
 * layers whose own list was kept because the heuristic returned nobody.  The append of absent keys reports to
 * hnsw_index_build_stats. */
int hnsw_index_update_stats(const hnsw_index_t *index, int64_t *rounds, int64_t *relinks, int64_t *relinks_superseded,
                            int64_t *additions_already_present, int64_t *distance_evals, int64_t *lists_kept);
/* Room for `capacity` rows without reallocating the per-row buffers (capacity below the current room: nothing happens; it never
 * shrinks).  The rows of the upper layers, about one per maxM rows, still grow by 1.5x. */
int hnsw_index_reserve(hnsw_index_t *index, int64_t capacity);
/* Counters of the last device build or append of this index (any pointer may be NULL): rounds run, additions a re-selection did
 * not see, candidate-queue prunes, candidates dropped because a pruned queue was still full. */
int hnsw_index_build_stats(const hnsw_index_t *index, int64_t *rounds, int64_t *unseen_additions, int64_t *queue_prunes,
                           int64_t *dropped_candidates);
int hnsw_index_graph_size(const hnsw_index_t *index, int64_t *n_entries, int64_t *n_neighbours, int64_t *entry_point,
                          int32_t *max_level);
int hnsw_index_graph(const hnsw_index_t *index, int32_t *entry_level, int64_t *entry_item, int64_t *entry_offsets,
                     int64_t *entry_neighbours);
/* n vectors of dimension d, the metric and maxM the index was created with; the keys searches return (positions
 * when the index was given no ids) */
int hnsw_index_info(const hnsw_index_t *index, int64_t *n, int32_t *d, int32_t *metric, int32_t *max_m);
int hnsw_index_get_ids(const hnsw_index_t *index, int64_t *out);
int hnsw_index_get_vectors(const hnsw_index_t *index, int64_t i0, int64_t n, float *out);
int hnsw_index_destroy(hnsw_index_t *index);

/* searchKnn for nq queries (row-major fp32 [nq][d]): out_dist / out_ids [nq][k] ascending by distance,
 * out_counts[nq] = neighbours found (<= k).  ef as HnswParams.ef; the beam is max(ef, k) (HnswIndex.java:545).
 * max(ef, k) <= 1024. */
int hnsw_search(hnsw_index_t *index, int32_t nq, const float *queries, int32_t k, int32_t ef, float *out_dist,
                int64_t *out_ids, int32_t *out_counts);

/* Work counters of the last hnsw_search: distance evaluations, layer-0 expansions, queries that needed the
 * global-memory queues, and the kernel time (HIP events, ms). */
int hnsw_last_stats(const hnsw_index_t *index, int64_t *distance_evals, int64_t *expansions, int32_t *spilled_queries,
                    float *kernel_ms);
/* More counters of the last hnsw_search: neighbours admitted to the queues (each costs an offer to both queues and, once the
 * result queue is full, a poll), and the largest candidate queue any query of the batch reached. */
int hnsw_last_walk_counters(const hnsw_index_t *index, int64_t *admissions, int64_t *largest_candidate_queue);

#ifdef __cplusplus
}
#endif
#endif
