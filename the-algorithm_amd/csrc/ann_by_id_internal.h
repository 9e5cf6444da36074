// ann_by_id_internal.h -- the seam between the by-id queries (ann_by_id.hip) and the two dense indexes.
//
// hnsw_search and dann_search are each "upload + prepare" followed by "search the prepared device queries"; the second halves
// are the *_search_prepared functions below, which the by-id entry points share with the plain searches.  The first halves of
// a by-id query (resolve, gather + prepare) live in ann_by_id.hip and write straight into the buffers *_open hands out.
// Every function returns the owning module's status code and leaves its message in that module's *_last_error().
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>

struct hnsw_index;
struct dann_index;
struct ann_store;

namespace ann_by_id {

// A built store as the by-id queries of the inverted-file family read it (faiss_by_id.hip): the (key, position) table sorted
// by key and the fp32 rows [n][d], all on `device`.  The pointers live as long as the store.
struct StoreView {
  int device = 0, d = 0;
  int64_t n = 0;
  const int64_t *keys = nullptr, *kpos = nullptr;
  const float *rows = nullptr;
};
int store_view(const ann_store *store, StoreView *out);

// What the index shows of itself: where prepared queries go, and (own_keys) its rows and key -> position table as a producer.
struct HnswTarget {
  int device = 0, metric = 0, d = 0, dpad = 0;
  int64_t n = 0;
  bool empty = false;             // no entry point: every search answers nothing
  _Float16 *q = nullptr;          // prepared queries [nq_cap][dpad]
  const _Float16 *x = nullptr;    // stored rows [n][dpad]
  const int64_t *kp_keys = nullptr, *kp_pos = nullptr;  // (key, position) sorted by key; NULL: keys are positions
  int64_t kp_n = 0;
};
struct DeviceResult {
  const float *dist = nullptr;    // [nq][k]
  const int64_t *ids = nullptr;   // [nq][k]
  const int32_t *counts = nullptr;
  int64_t h2d_bytes = 0, d2h_bytes = 0;  // control traffic of the search itself
};

// Refuses what hnsw_search refuses (k, ef, a broken index), reserves the prepared-query buffer for nq_cap rows and, with
// own_keys, brings the index's (key, position) table up to date.
int hnsw_open(hnsw_index *ix, int32_t nq_cap, int32_t k, int32_t ef, bool own_keys, HnswTarget *out);
// The walks over the first nq rows of the prepared-query buffer, second pass included; ends synchronised, results on the device.
int hnsw_search_prepared(hnsw_index *ix, int32_t nq, int32_t k, int32_t ef, DeviceResult *out);
std::shared_ptr<void> &hnsw_scratch(hnsw_index *ix);  // the by-id scratch of this index (freed with it)

struct DannTarget {
  int device = 0, metric = 0, d = 0, S = 0;
  int64_t n = 0;
  bool exact = false;
  const _Float16 *xf = nullptr;   // stored fragments
  const int64_t *kp_keys = nullptr, *kp_pos = nullptr;
  int64_t kp_n = 0;
};
struct DannChunk {
  _Float16 *qf = nullptr;         // query fragments of the chunk (zeroed)
  float *qsumsq = nullptr;        // [nq_pad]
  float *q_in = nullptr;          // [nq][d] fp32 queries: read by the exact mode's second scoring only
};
constexpr int DANN_CHUNK = 4096;  // queries per dann search chunk (dense_ann.hip MAX_NQ)

int dann_open(dann_index *ix, int32_t k, bool own_keys, DannTarget *out);
// One chunk of <= DANN_CHUNK queries: reserve and reset the per-search buffers, then (after the caller has prepared the
// queries into them) the GEMM passes, re-arm rounds and selection into the given device outputs; ends synchronised.
int dann_chunk_open(dann_index *ix, int32_t nq, int32_t k, DannChunk *out);
int dann_chunk_search_prepared(dann_index *ix, int32_t nq, int32_t k, float *o_dist, int64_t *o_ids, int32_t *o_cnt,
                               int64_t *d2h_bytes);
std::shared_ptr<void> &dann_scratch(dann_index *ix);
// dann_index_build without ids from rows that are on the device already (row-major fp32 [n][d]): the coarse quantizer of
// ivf_ann.hip rebuilds its centroid index this way in every k-means round.  Free with dann_index_destroy.
// stored: the rows are values an index stored before (fp16 values, Cosine rows normalised already); they are kept as they
// are -- a Cosine index does not normalise them again, which could move a rounded value by an ulp.
int dann_build_device(int32_t device, int32_t metric, int64_t n, int32_t d, const float *d_rows, dann_index **out,
                      bool stored = false);

}  // namespace ann_by_id
