// ivf_hnsw_quantizer.hip -- include/ivf_hnsw_quantizer.h: the HNSW coarse quantizer of the inverted-file indexes.
//
// This source makes, replaces and frees the graph; the walk itself is the inverted-file core's coarse step (ivf_core.h:
// assign_rows, probe_chunk) over the seam of ann_by_id_internal.h.  Every entry point dispatches on `kind` to the hook of
// the index source (ivf_hnsw_quantizer_internal.h), which hands out the index's quantizer state; the graph is an
// hnsw_index over the stored centroids, built or loaded by hnsw_ann.hip's own constructors.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/dense_ann.h"
#include "../../include/faiss_files.h"
#include "../../include/hnsw_ann.h"
#include "../../include/ivf_ann.h"
#include "../../include/ivf_hnsw_quantizer.h"
#include "faiss_restore.h"
#include "ivf_error.h"
#include "ivf_hnsw_quantizer_internal.h"

namespace {

// the quantizer state of the index behind (kind, index); NULL with the message set
ivf_hq::State *state_of(int32_t kind, const void *index) {
  if (!index) {
    (void)fail(IVF_EINVAL, "null index");
    return nullptr;
  }
  void *ix = const_cast<void *>(index);
  switch (kind) {
    case FAISS_KIND_IVF_FLAT: return ivf_internal::hnsw_quantizer((ivf_index *)ix);
    case FAISS_KIND_IVF_PQ: return ivfpq_internal::hnsw_quantizer((ivfpq_index *)ix);
    case FAISS_KIND_OPQ_IVF_PQ: return ivfpq_internal::hnsw_quantizer(opq_internal::inner((opq_index *)ix));
  }
  (void)fail(IVF_EINVAL, "unknown index kind " + std::to_string(kind) + " (1: IVF-Flat, 2: IVF-PQ, 3: OPQ)");
  return nullptr;
}

int graph_metric(const ivf_hq::State *s) { return s->metric == IVF_METRIC_L2 ? HNSW_METRIC_L2 : HNSW_METRIC_INNER_PRODUCT; }

// the stored centroids on the host, fp32 [nlist][d]
int stored_centroids(const ivf_hq::State *s, std::vector<float> &out) {
  out.resize((size_t)s->nlist * s->d);
  if (int rc = dann_index_get_vectors(s->coarse, 0, s->nlist, out.data()))
    return fail(rc, std::string("centroids: ") + dann_last_error());
  return IVF_OK;
}

// the index takes the new graph; the one it held goes
void install(ivf_hq::State *s, hnsw_index_t *graph, int max_m) {
  if (s->graph) (void)hnsw_index_destroy(s->graph);
  s->graph = graph;
  s->max_m = max_m;
  s->ef = ivf_hq::DEFAULT_EF;
  s->evals = s->expansions = s->missing = 0;
  s->last_q_n = 0;
}

}  // namespace

extern "C" {

const char *ivfhq_last_error(void) { return g_err.c_str(); }

int ivfhq_build(int32_t kind, void *index, int32_t max_m, int32_t ef_construction, uint64_t seed, int32_t batch) try {
  ivf_hq::State *s = state_of(kind, index);
  if (!s) return IVF_EINVAL;
  std::vector<float> cent;
  if (int rc = stored_centroids(s, cent)) return rc;
  hnsw_index_t *graph = nullptr;
  if (int rc = hnsw_index_build_insert_gpu(s->device, graph_metric(s), s->nlist, s->d, cent.data(), nullptr, max_m, ef_construction,
                                           seed, batch, &graph))
    return fail(rc, std::string("graph build: ") + hnsw_last_error());
  install(s, graph, max_m);
  return IVF_OK;
} ABI_CATCH

int ivfhq_attach_graph(int32_t kind, void *index, int32_t max_m, int64_t entry_point, int32_t max_level, int64_t n_entries,
                       const int32_t *entry_level, const int64_t *entry_item, const int64_t *entry_offsets,
                       const int64_t *entry_neighbours) try {
  ivf_hq::State *s = state_of(kind, index);
  if (!s) return IVF_EINVAL;
  if (entry_point < 0) return fail(IVF_EINVAL, "the graph has no entry point: a quantizer must reach at least one cell");
  std::vector<float> cent;
  if (int rc = stored_centroids(s, cent)) return rc;
  hnsw_index_t *graph = nullptr;
  if (int rc = hnsw_index_build(s->device, graph_metric(s), s->nlist, s->d, cent.data(), nullptr, max_m, entry_point, max_level,
                                n_entries, entry_level, entry_item, entry_offsets, entry_neighbours, &graph))
    return fail(rc, std::string("graph: ") + hnsw_last_error());
  install(s, graph, max_m);
  return IVF_OK;
} ABI_CATCH

int ivfhq_detach(int32_t kind, void *index) try {
  ivf_hq::State *s = state_of(kind, index);
  if (!s) return IVF_EINVAL;
  install(s, nullptr, 0);
  return IVF_OK;
} ABI_CATCH

int ivfhq_set_ef(int32_t kind, void *index, int32_t quantizer_ef) try {
  if (quantizer_ef < 1 || quantizer_ef > ivf_hq::MAX_EF) return fail(IVF_EINVAL, "quantizer_ef must be in 1..1024");
  ivf_hq::State *s = state_of(kind, index);
  if (!s) return IVF_EINVAL;
  if (!s->graph) return fail(IVF_EINVAL, "the index has no HNSW quantizer: quantizer_ef has nothing to set");
  s->ef = quantizer_ef;
  return IVF_OK;
} ABI_CATCH

int ivfhq_info(int32_t kind, const void *index, int32_t *attached, int32_t *max_m, int32_t *quantizer_ef) try {
  const ivf_hq::State *s = state_of(kind, index);
  if (!s) return IVF_EINVAL;
  if (attached) *attached = s->graph ? 1 : 0;
  if (max_m) *max_m = s->max_m;
  if (quantizer_ef) *quantizer_ef = s->ef;
  return IVF_OK;
} ABI_CATCH

int ivfhq_quantizer(int32_t kind, void *index, hnsw_index_t **borrowed) try {
  ivf_hq::State *s = state_of(kind, index);
  if (!s) return IVF_EINVAL;
  if (!borrowed) return fail(IVF_EINVAL, "null argument");
  *borrowed = s->graph;
  return IVF_OK;
} ABI_CATCH

int ivfhq_last_queries(int32_t kind, const void *index, int32_t *nq, int32_t *d, float *out) try {
  const ivf_hq::State *s = state_of(kind, index);
  if (!s) return IVF_EINVAL;
  if (nq) *nq = s->last_q_n;
  if (d) *d = s->d;
  if (out && s->last_q_n > 0) {
    const size_t count = (size_t)s->last_q_n * s->d;
    std::vector<_Float16> h(count);
    ITRY(hipSetDevice(s->device));
    ITRY(hipMemcpy(h.data(), s->last_q, count * sizeof(_Float16), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < count; ++i) out[i] = (float)h[i];
  }
  return IVF_OK;
} ABI_CATCH

int ivfhq_last_stats(int32_t kind, const void *index, int64_t *distance_evals, int64_t *expansions, int64_t *missing_probes) try {
  const ivf_hq::State *s = state_of(kind, index);
  if (!s) return IVF_EINVAL;
  if (distance_evals) *distance_evals = s->evals;
  if (expansions) *expansions = s->expansions;
  if (missing_probes) *missing_probes = s->missing;
  return IVF_OK;
} ABI_CATCH

}  // extern "C"
