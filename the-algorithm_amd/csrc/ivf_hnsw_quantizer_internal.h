// ivf_hnsw_quantizer_internal.h -- the seam between include/ivf_hnsw_quantizer.h (ivf_hnsw_quantizer.hip) and the three
// inverted-file indexes.
//
// The inverted-file core (ivf_core.h) holds one ivf_hq::State per index: the optional HNSW graph over the centroids, its
// quantizer_ef and what the last search's walks left.  With `graph` NULL the core's coarse step is the exhaustive search it
// always was.  ivf_hnsw_quantizer.hip builds, attaches and frees the graph through the pointer a hook hands out; the core
// reads it in assign_rows and probe_chunk and frees it with the index.  An OPQ index is reached through its inner IVF-PQ
// index (opq_internal::inner, faiss_restore.h).  None of these is an exported symbol of the library.
#pragma once
#include <cstdint>

struct hnsw_index;
struct dann_index;
struct ivf_index;
struct ivfpq_index;

namespace ivf_hq {

constexpr int DEFAULT_EF = 16;  // Faiss: HNSW::efSearch
constexpr int MAX_EF = 1024;

struct State {
  // what the index shows of itself (filled by the hook)
  int device = 0, metric = 0, d = 0, nlist = 0;
  const dann_index *coarse = nullptr;  // the stored centroids
  // the quantizer: items are cells, vectors the stored centroids; L2 -> L2, InnerProduct and Cosine -> InnerProduct
  hnsw_index *graph = nullptr;
  int max_m = 0;
  int ef = DEFAULT_EF;
  // the last search: the walks' counters summed over its chunks, and its prepared queries (fp16 [last_q_n][d], device)
  int64_t evals = 0, expansions = 0, missing = 0;
  const void *last_q = nullptr;
  int32_t last_q_n = 0;
};

}  // namespace ivf_hq

namespace ivf_internal __attribute__((visibility("hidden"))) {
ivf_hq::State *hnsw_quantizer(ivf_index *ix);
}
namespace ivfpq_internal __attribute__((visibility("hidden"))) {
ivf_hq::State *hnsw_quantizer(ivfpq_index *ix);
}
