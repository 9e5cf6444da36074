// ivf_device_rows.h -- the seam between the OPQ pre-transform (opq_ann.hip), the shard set (shard_set.hip), the by-id queries
// (faiss_by_id.hip) and the inverted-file indexes.
//
// ivf_index_train, ivfpq_index_train, ivfpq_index_add and ivfpq_search are each "bring host rows to the device" followed
// by work on device rows; the second halves are the functions below, which the public entry points share with
// opq_ann.hip, whose transformed rows, queries and training set are on the device already and never cross to the host.
// Every function returns the owning module's status code and leaves its message in that module's *_last_error().
// None of these is an exported symbol of the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>

struct ivf_index;
struct ivfpq_index;
struct ivfsq_index;
struct shardset;

namespace ivf_internal __attribute__((visibility("hidden"))) {

// ivf_index_train over training rows that are on the device (row-major fp32 [n_train][d]).
int train_device(int32_t device, int32_t metric, int32_t d, int32_t nlist, int64_t n_train, const float *d_rows, int32_t niter,
                 uint64_t seed, ivf_index **out);

// ivf_search over queries that are on the device, the answer left in the caller's device buffers d_dist / d_ids [nq][k] and
// d_counts [nq] by the select launch itself (slots past a count are zeros, as ivf_search leaves them): nothing but control
// words (round flags, the rows counter, the two group counts) leaves the device.  The bytes are ivf_search's.
int search_device_out(ivf_index *ix, int32_t nq, const float *d_queries, int32_t k, int32_t nprobe, float *d_dist, int64_t *d_ids,
                      int32_t *d_counts);
// search_device_out over rows of a device-resident store read through a position list: query i is the fp32 row
// d_store_rows + d_pos[i] * d (a by-id query, include/faiss_by_id.h; every position is inside the store).  The rows are
// prepared where they lie (ivf_kernels.h: store_rows_pos_kernel), with no fp32 copy in between; the bytes are ivf_search's
// over a copy of the rows.  The same entry exists below for every member of the family.
int search_store_out(ivf_index *ix, int32_t nq, const float *d_store_rows, const int64_t *d_pos, int32_t k, int32_t nprobe,
                     float *d_dist, int64_t *d_ids, int32_t *d_counts);
int device_of(const ivf_index *ix);
// the control bytes the last search moved (answers not counted), and the part of them that went up (an HNSW quantizer's
// second-pass query list; 0 for the exhaustive quantizer)
int64_t last_control_bytes(const ivf_index *ix);
int64_t last_control_upload_bytes(const ivf_index *ix);
std::shared_ptr<void> &by_id_scratch(ivf_index *ix);  // the by-id scratch of this index (freed with it)

}  // namespace ivf_internal

namespace ivfsq_internal __attribute__((visibility("hidden"))) {

// ivfsq_search over queries that are on the device, or over rows of a store (as ivf_internal's two above), the answer left
// in the caller's device buffers.
int search_device_out(ivfsq_index *ix, int32_t nq, const float *d_queries, int32_t k, int32_t nprobe, float *d_dist, int64_t *d_ids,
                      int32_t *d_counts);
int search_store_out(ivfsq_index *ix, int32_t nq, const float *d_store_rows, const int64_t *d_pos, int32_t k, int32_t nprobe,
                     float *d_dist, int64_t *d_ids, int32_t *d_counts);
int device_of(const ivfsq_index *ix);
int64_t last_control_bytes(const ivfsq_index *ix);
int64_t last_control_upload_bytes(const ivfsq_index *ix);
std::shared_ptr<void> &by_id_scratch(ivfsq_index *ix);

}  // namespace ivfsq_internal

namespace ivfpq_internal __attribute__((visibility("hidden"))) {

// ivfpq_index_train over training rows that are on the device.
int train_device(int32_t device, int32_t metric, int32_t d, int32_t nlist, int32_t M, int64_t n_train, const float *d_rows,
                 int32_t niter, uint64_t seed, ivfpq_index **out);

// ivfpq_index_train_polysemous (polysemous_ann.h) over training rows that are on the device.
int train_device_polysemous(int32_t device, int32_t metric, int32_t d, int32_t nlist, int32_t M, int64_t n_train, const float *d_rows,
                            int32_t niter, uint64_t seed, int64_t anneal_iters, ivfpq_index **out);

// ivfpq_index_add in three steps.  add_begin refuses what ivfpq_index_add refuses (n > 0) and makes room for n rows;
// add_slab prepares, assigns and encodes rows [r0, r0 + m) of the add from device rows (row-major fp32 [m][d]; m at most
// slab_rows()); add_end takes the ids (host, or NULL), counts the rows in and lays the lists out again.  The index is
// unchanged until add_end.
int add_begin(ivfpq_index *ix, int64_t n, bool with_ids);
int add_slab(ivfpq_index *ix, int64_t r0, int64_t m, const float *d_rows);
int add_end(ivfpq_index *ix, int64_t n, const int64_t *ids);
int64_t slab_rows(int d);  // rows of dimension d in a 64-MiB fp32 slab

// ivfpq_search over queries that are on the device (row-major fp32 [nq][d]); the outputs are host buffers.
int search_device(ivfpq_index *ix, int32_t nq, const float *d_queries, int32_t k, int32_t nprobe, float *out_dist,
                  int64_t *out_ids, int32_t *out_counts);

// ivfpq_search_ht (polysemous_ann.h) over queries that are on the device; ht <= 0 is search_device.
int search_device_ht(ivfpq_index *ix, int32_t nq, const float *d_queries, int32_t k, int32_t nprobe, int32_t ht, float *out_dist,
                     int64_t *out_ids, int32_t *out_counts);

// search_device_ht with the answer left in the caller's device buffers, as ivf_internal::search_device_out leaves it.
int search_device_out(ivfpq_index *ix, int32_t nq, const float *d_queries, int32_t k, int32_t nprobe, int32_t ht, float *d_dist,
                      int64_t *d_ids, int32_t *d_counts);
int search_store_out(ivfpq_index *ix, int32_t nq, const float *d_store_rows, const int64_t *d_pos, int32_t k, int32_t nprobe,
                     int32_t ht, float *d_dist, int64_t *d_ids, int32_t *d_counts);
int64_t last_control_bytes(const ivfpq_index *ix);
int64_t last_control_upload_bytes(const ivfpq_index *ix);
std::shared_ptr<void> &by_id_scratch(ivfpq_index *ix);

// After a search_device that stood in for a search with ht <= 0: every scanned row counts as scored (ivfpq_last_ht_stats).
int search_stats_unfiltered(ivfpq_index *ix);

// search_device with the select step writing, instead of the answer, what the re-rank of refine_ann.hip needs: for query q
// its candidates best first by (distance, id) as add-order positions d_pos[q * k ..] (-1 past the count), their ranks in
// (id, position) order d_rank[q * k ..] and their number d_counts[q].  All three are device buffers; nothing but the scan's
// round flags leaves the device.  The last-search exports of the index (probes, stats) describe this search.
int search_positions(ivfpq_index *ix, int32_t nq, const float *d_queries, int32_t k, int32_t nprobe, int32_t *d_pos,
                     uint32_t *d_rank, int32_t *d_counts);
// The ids in (id, position) order on the device, [n]: ids_sorted[rank] is the id of the candidate of that rank.
const int64_t *device_ids_sorted(const ivfpq_index *ix);
int device_of(const ivfpq_index *ix);  // the device the index lives on

// A product quantiser on the rows themselves (no coarse quantizer, no residuals): M sub-quantizers of 256 codewords over
// n fp16 device rows [n][d], by the encoder and the mean kernel of the index with one all-zero centroid and every row in
// cell 0.  init: the initial codewords are picked by the rule of ivfpq_ann.h with this seed; otherwise d_cb holds them.
// Then `rounds` Lloyd rounds, then the final encoding into d_codes (uint8 [n][M]).  d_cb: fp32 [M][256][d / M].
int pq_train_plain(int32_t device, const _Float16 *d_rows16, int64_t n, int32_t d, int32_t M, bool init, int32_t rounds,
                   uint64_t seed, float *d_cb, uint8_t *d_codes);

}  // namespace ivfpq_internal

struct opq_index;

namespace opq_internal __attribute__((visibility("hidden"))) {

// opq_index_add over rows that are on the device (row-major fp32 [m][d_in], not yet prepared): add_begin and add_end are
// those of the inner index (faiss_restore.h's inner()); add_slab transforms rows [r0, r0 + m) of the add, m at most
// slab_rows(), and hands them to the inner add_slab.
int add_slab(opq_index *ix, int64_t r0, int64_t m, const float *d_rows);
int64_t slab_rows(const opq_index *ix);
// ivfpq_internal::search_positions over device queries [nq][d_in], which are prepared and transformed first.
int search_positions(opq_index *ix, int32_t nq, const float *d_queries, int32_t k, int32_t nprobe, int32_t *d_pos,
                     uint32_t *d_rank, int32_t *d_counts);
// opq_search_ht over device queries [nq][d_in] (prepared and transformed on the device, no staging copy), the answer left
// in the caller's device buffers as ivf_internal::search_device_out leaves it.
int search_device_out(opq_index *ix, int32_t nq, const float *d_queries, int32_t k, int32_t nprobe, int32_t ht, float *d_dist,
                      int64_t *d_ids, int32_t *d_counts);
// search_device_out over rows of a store [.][d_in] read through a position list: the transform's tile load goes through
// the list (opq_transform_kernel<true>), its output feeds the inner index's device search as above.
int search_store_out(opq_index *ix, int32_t nq, const float *d_store_rows, const int64_t *d_pos, int32_t k, int32_t nprobe,
                     int32_t ht, float *d_dist, int64_t *d_ids, int32_t *d_counts);
int device_of(const opq_index *ix);
int64_t last_control_bytes(const opq_index *ix);
int64_t last_control_upload_bytes(const opq_index *ix);
std::shared_ptr<void> &by_id_scratch(opq_index *ix);

}  // namespace opq_internal

namespace shardset_internal __attribute__((visibility("hidden"))) {

// shardset_search over rows of a store [.][dimension] read through a position list, the answer left in the caller's device
// buffers d_dist / d_ids [nq][k] and d_counts [nq]: a chunk's rows are copied once into the set's query buffer, in the
// layout shardset_search uploads, and every member searches them there.  Refuses what shardset_search refuses; the
// set's last stats describe this search (its upload is 0).
int search_store_out(shardset *set, int32_t nq, const float *d_store_rows, const int64_t *d_pos, int32_t k, int32_t nprobe,
                     int32_t ht, float *d_dist, int64_t *d_ids, int32_t *d_counts);
// ht > 0 with an IVF-Flat member: the refusal of shardset_search, before any device work
int check_ht(const shardset *set, int32_t ht);
int device_of(const shardset *set);
int dimension_of(const shardset *set);
int64_t last_control_bytes(const shardset *set);
int64_t last_control_upload_bytes(const shardset *set);
std::shared_ptr<void> &by_id_scratch(shardset *set);

}  // namespace shardset_internal
