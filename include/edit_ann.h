/*
 * edit_ann.h -- C ABI of the exhaustive index under the EditDistance metric, MI355X (gfx950).
 *
 * What it serves: the fourth metric of the reference's ann/ (paths relative to ann/src/main/):
 *   scala/com/twitter/ann/common/Metric.scala:63-73      Metric.fromString accepts "EditDistance"
 *   scala/com/twitter/ann/common/Metric.scala:187-261    Metric.Edit: Levenshtein distance with unit costs over Seq[Float]
 *   thrift/com/twitter/ann/common/ann_common.thrift:16-19    DistanceMetric.EditDistance = 7
 *   thrift/com/twitter/ann/common/ann_common.thrift:107-121  Distance.editDistance, arm 4: a struct with field 1, an i32
 *   scala/com/twitter/ann/brute_force/BruteForceIndex.scala:40-91   append and queryWithDistance, generic over the metric
 *
 * Semantics
 *   distance   insert, delete and substitute cost 1 each; two elements are equal when Scala's Float == says so, which is IEEE
 *              equality: -0.0 equals 0.0, a NaN equals nothing (itself included), an infinity equals itself, denormals are
 *              ordinary values.  An empty string is at distance len(other).  A distance is an int32.
 *   search     the k nearest of every query, ordered by (distance ascending, id ascending); rows with one id order by the
 *              position at which they arrived.  out_counts[q] = min(k, n); the entries past it hold distance -1 and id -1.
 *   append     a search on build(X0) + append(X1) + ... returns the bytes of a search on build(X0 ++ X1 ++ ...).
 *   strings    travel as CSR: row i is chars[offsets[i] .. offsets[i + 1]), one fp32 per character.  Every function that takes
 *              a CSR pair also takes n_chars, the number of elements of `chars`, and checks the offsets against it:
 *              0 <= offsets[0], offsets non-decreasing, offsets[n] <= n_chars.
 *
 * Limits, refused by name and never clipped
 *   a string has 0..256 elements, stored rows and queries alike: more is EDIT_ELIMIT
 *   1 <= k <= 1024, else EDIT_EINVAL
 *   an index holds fewer than 2^31 - 64 rows: more is EDIT_ELIMIT
 *   nq is unbounded: a batch is answered in slices sized from the scratch budget (edit_index_set_query_slice)
 *   there is no data-dependent refusal: any number of rows may tie at any distance.  Distances lie in 0..256, so the
 *   selection counts (a 257-bin histogram per query, a threshold, an ordered compaction) and has no survivor cap.
 *
 * Where the rows live: the index keeps the rows on the host in arrival order and lays them on the device, 64 rows to a tile
 * in (id, position) order, at the first search after they arrived.  An append whose ids are all at or above the largest
 * stored id (always so without ids) lays only its own tiles; any other append re-sorts and re-lays the whole index at the
 * next search, O(n).  Building and appending touch no device, so a wrong `device` is reported (EDIT_EDEVICE) by the first
 * search.
 *
 * Out of scope: HNSW under this metric (the walk of hnsw_ann.h restates a float-keyed priority queue; an integer-distance
 * walk needs a restatement of its own -- this index is its truth set and edit_pair_distances its distance core),
 * BruteForceFileData serialisation, JNI, QueryableById, shard sets and grouped membership, and case folding (the reference
 * only muses about it in a comment, Metric.scala:204-205).
 *
 * No function throws or aborts; every function returns a status, and edit_last_error() has the message of the last failure
 * on the calling thread.  One call at a time per index.
 */
#ifndef EDIT_ANN_H
#define EDIT_ANN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define EDIT_OK 0
#define EDIT_EINVAL 1
#define EDIT_EDEVICE 2
#define EDIT_ELIMIT 3    /* a string longer than 256 elements, or 2^31 - 64 rows or more */
#define EDIT_ENOMEM 4    /* host allocation failed */
#define EDIT_EINTERNAL 5 /* an unexpected C++ exception was caught at the ABI; the message says which */
#define EDIT_ESPACE 6    /* wire encoder / decoder: the caller's buffer is too small (the needed size is reported) */
#define EDIT_EFORMAT 7   /* wire decoder: the bytes are not a NearestNeighborResult, or end inside a value */

#define EDIT_DISTANCE_METRIC 7 /* DistanceMetric.EditDistance, ann_common.thrift:16-19 */
#define EDIT_MAX_LENGTH 256
#define EDIT_MAX_K 1024

typedef struct edit_index edit_index_t;

const char *edit_last_error(void);

/* Build from n rows; ids NULL = the ids are the positions 0..n-1 (and every later append must pass NULL too).  n = 0 is a
 * valid empty index (offsets and chars may then be NULL). */
int edit_index_build(int32_t device, int64_t n, const int64_t *offsets, const float *chars, int64_t n_chars, const int64_t *ids,
                     edit_index_t **out);
/* BruteForceIndex.append for n more rows.  An index built with ids needs ids, one built without needs NULL: otherwise, and on
 * any other refusal, EDIT_EINVAL / EDIT_ELIMIT with the index unchanged. */
int edit_index_append(edit_index_t *index, int64_t n, const int64_t *offsets, const float *chars, int64_t n_chars, const int64_t *ids);
/* Host room for `rows` rows and `total_chars` elements in all, so that appends up to there do not reallocate; never shrinks. */
int edit_index_reserve(edit_index_t *index, int64_t rows, int64_t total_chars);
/* Any pointer may be NULL. */
int edit_index_info(const edit_index_t *index, int64_t *n, int64_t *total_chars, int32_t *max_len);
/* Audit: rows i0 .. i0 + n in arrival order, back as CSR: offsets [n + 1] starting at 0, chars (cap_chars elements of room;
 * too little is EDIT_ESPACE and *n_chars says how much is needed; chars NULL asks for the size only) with the very bits that
 * were stored, and ids [n] (may be NULL). */
int edit_index_get_rows(const edit_index_t *index, int64_t i0, int64_t n, int64_t *offsets, float *chars, int64_t cap_chars,
                        int64_t *n_chars, int64_t *ids);
void edit_index_destroy(edit_index_t *index);

/* queryWithDistance for nq queries: out_dist int32 [nq][k], out_ids int64 [nq][k], out_counts int32 [nq]. */
int edit_search(edit_index_t *index, int64_t nq, const int64_t *q_offsets, const float *q_chars, int64_t n_q_chars, int32_t k,
                int32_t *out_dist, int64_t *out_ids, int32_t *out_counts);

/* Metric.Edit.distance for n_pairs pairs (a[i], b[i]) on the device, through the device distance function of edit_search
 * (a is the pattern, b the text): out int32 [n_pairs]. */
int edit_pair_distances(int32_t device, int64_t n_pairs, const int64_t *a_offsets, const float *a_chars, int64_t n_a_chars,
                        const int64_t *b_offsets, const float *b_chars, int64_t n_b_chars, int32_t *out);
/* The same on the host and with no device call: the plain two-row dynamic programme, cell for cell what
 * Metric.scala:189-220 computes.  Safe to call from many threads at once. */
int edit_pair_distances_host(int64_t n_pairs, const int64_t *a_offsets, const float *a_chars, int64_t n_a_chars,
                             const int64_t *b_offsets, const float *b_chars, int64_t n_b_chars, int32_t *out);

/* Test knob: answer a batch in passes of at most this many queries (0 = automatic, from a 256 MiB scratch budget and the
 * row count, 4096 at most).  The answers do not depend on it. */
int edit_index_set_query_slice(edit_index_t *index, int32_t max_queries_per_pass);
/* HIP-event times of the last search, summed over its passes: the distance kernel, and everything that selects. */
int edit_last_timing(const edit_index_t *index, float *distance_ms, float *select_ms);
/* The last search: pairs = nq * n scored, and cell_updates = the sum over them of len(query) * len(row). */
int edit_last_stats(const edit_index_t *index, int64_t *pairs, int64_t *cell_updates);

/* NearestNeighborResult (ann_common.thrift:107-125) in TBinaryProtocol with the editDistance arm: every neighbour is
 * { 1: binary id (8 bytes, big-endian long), 2: Distance { 4: EditDistance { 1: i32 distance } } }; distances NULL leaves
 * field 2 out.  *len is the size needed even when cap is too small (EDIT_ESPACE). */
int edit_wire_encode_neighbor_result(int32_t count, const int64_t *ids, const int32_t *distances, uint8_t *buf, int64_t cap,
                                     int64_t *len);
/* arms[i] = 4 where the neighbour carried an editDistance, 0 where it carried no distance or another arm (its distance is
 * then 0).  *count is the number of neighbours in the message even when cap is smaller (EDIT_ESPACE). */
int edit_wire_decode_neighbor_result(const uint8_t *buf, int64_t n, int32_t cap, int64_t *ids, int32_t *distances, int32_t *arms,
                                     int32_t *count, int64_t *consumed);

#ifdef __cplusplus
}
#endif
#endif
