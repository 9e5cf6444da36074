// faiss_restore.h -- the seam between the index files (faiss_files.cpp, host code) and the three inverted-file indexes.
//
// A built index leaves the process as the state it exports and comes back as exactly that state: the stored centroids, the
// codebooks, the matrix and, per row in the order added, the id, the cell and the payload (the stored fp16 row of an
// IVF-Flat index, the M code bytes of an IVF-PQ index).  Nothing is assigned, encoded or trained on the way in, and no
// value is rounded or normalised again.
//
//   restore_begin   a new index over the given stored values, with room for n rows; it holds no row yet
//   restore_stage   pinned host memory for the next slab of at most restore_slab_rows() rows: the file is read into it
//   restore_slab    staging -> device at rows [r0, r0 + m); r0 continues where the last slab ended.  A validation kernel
//                   then checks the slab (every cell in [0, nlist); ids-are-positions: every id equals its position) and
//                   reports the first offending row through a flag word: IVF_EINVAL.  Nothing has indexed by a loaded
//                   value at that point, and the caller destroys the index.
//   restore_end     all n rows are in: the lists are laid out once, by the layout an add uses
//   export_rows     rows [r0, r0 + m) as stored, in the order added (any of the outputs may be NULL)
//
// Every function returns the owning module's status code and leaves its message in that module's *_last_error().
// None of these is an exported symbol of the library.  No HIP type appears here: the file code is compiled as host C++.
#pragma once
#include <cstdint>

struct ivf_index;
struct ivfpq_index;
struct opq_index;

namespace ivf_internal __attribute__((visibility("hidden"))) {

int64_t restore_slab_rows(int32_t d);
// centroids: host fp32 [nlist][d], the values ivf_index_get_centroids gave.  ids_mode: -1 (n = 0), 0 positions, 1 given.
int restore_begin(int32_t device, int32_t metric, int32_t d, int32_t nlist, const float *centroids, int32_t ids_mode, int64_t n,
                  ivf_index **out);
int restore_stage(ivf_index *ix, int64_t m, int64_t **ids, int32_t **cells, uint16_t **rows16);
int restore_slab(ivf_index *ix, int64_t r0, int64_t m);
int restore_end(ivf_index *ix);
int export_rows(const ivf_index *ix, int64_t r0, int64_t m, int64_t *ids, int32_t *cells, uint16_t *rows16);
int ids_mode(const ivf_index *ix);

}  // namespace ivf_internal

namespace ivfpq_internal __attribute__((visibility("hidden"))) {

int64_t restore_slab_rows(int32_t M);
// centroids as above; codebooks: host fp32 [M][256][d / M]
int restore_begin(int32_t device, int32_t metric, int32_t d, int32_t nlist, int32_t M, const float *centroids,
                  const float *codebooks, int32_t ids_mode, int64_t n, ivfpq_index **out);
int restore_stage(ivfpq_index *ix, int64_t m, int64_t **ids, int32_t **cells, uint8_t **codes);
int restore_slab(ivfpq_index *ix, int64_t r0, int64_t m);
int restore_end(ivfpq_index *ix);
int export_rows(const ivfpq_index *ix, int64_t r0, int64_t m, int64_t *ids, int32_t *cells, uint8_t *codes);
int ids_mode(const ivfpq_index *ix);

}  // namespace ivfpq_internal

namespace opq_internal __attribute__((visibility("hidden"))) {

// The transform with an inner index begun by ivfpq_internal::restore_begin (metric: that of the OPQ index; A: host fp32
// [d_out][d_in]).  The rows go through ivfpq_internal::restore_* on inner(); a failure there carries its message in
// ivfpq_last_error().
int restore_begin(int32_t device, int32_t metric, int32_t d_in, int32_t d_out, int32_t nlist, int32_t M, const float *A,
                  const float *centroids, const float *codebooks, int32_t ids_mode, int64_t n, opq_index **out);
ivfpq_index *inner(const opq_index *ix);

}  // namespace opq_internal
