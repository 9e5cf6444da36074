// ivf_device_rows.h -- the seam between the OPQ pre-transform (opq_ann.hip) and the two inverted-file indexes.
//
// ivf_index_train, ivfpq_index_train, ivfpq_index_add and ivfpq_search are each "bring host rows to the device" followed
// by work on device rows; the second halves are the functions below, which the public entry points share with
// opq_ann.hip, whose transformed rows, queries and training set are on the device already and never cross to the host.
// Every function returns the owning module's status code and leaves its message in that module's *_last_error().
// None of these is an exported symbol of the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct ivf_index;
struct ivfpq_index;

namespace ivf_internal __attribute__((visibility("hidden"))) {

// ivf_index_train over training rows that are on the device (row-major fp32 [n_train][d]).
int train_device(int32_t device, int32_t metric, int32_t d, int32_t nlist, int64_t n_train, const float *d_rows, int32_t niter,
                 uint64_t seed, ivf_index **out);

}  // namespace ivf_internal

namespace ivfpq_internal __attribute__((visibility("hidden"))) {

// ivfpq_index_train over training rows that are on the device.
int train_device(int32_t device, int32_t metric, int32_t d, int32_t nlist, int32_t M, int64_t n_train, const float *d_rows,
                 int32_t niter, uint64_t seed, ivfpq_index **out);

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

// A product quantiser on the rows themselves (no coarse quantizer, no residuals): M sub-quantizers of 256 codewords over
// n fp16 device rows [n][d], by the encoder and the mean kernel of the index with one all-zero centroid and every row in
// cell 0.  init: the initial codewords are picked by the rule of ivfpq_ann.h with this seed; otherwise d_cb holds them.
// Then `rounds` Lloyd rounds, then the final encoding into d_codes (uint8 [n][M]).  d_cb: fp32 [M][256][d / M].
int pq_train_plain(int32_t device, const _Float16 *d_rows16, int64_t n, int32_t d, int32_t M, bool init, int32_t rounds,
                   uint64_t seed, float *d_cb, uint8_t *d_codes);

}  // namespace ivfpq_internal
