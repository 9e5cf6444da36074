// refine_ann.hip -- re-ranking of the product-quantised indexes' answers by the stored rows (Faiss's IndexRefineFlat,
// `,RFlat`) for gfx950.
//
// What it replaces: ann_common.thrift:49-50 names the mechanism ("How many times more neighbours are requested from
// underlying index by IndexRefine"); FaissIndexer.scala:82-92 hands any factory string to index_factory.  The contract is
// include/refine_ann.h; the base is ivfpq_ann.hip or opq_ann.hip, reached device to device through ivf_device_rows.h: the
// candidates of a search never cross to the host.
//
// Shape of the computation.
//   * The store is fp16 [n][stride], stride = d rounded up to 8 halves (16 bytes), the padding zero.  An add prepares a slab
//     with store_rows_kernel (ivf_kernels.h: the preparation of every inverted-file index), copies it into the store
//     behind the rows that are there, and hands the same device rows to the base's add_slab; the base's add_end commits.
//   * A search asks the base's select step for positions (ivfpq_internal::search_positions) at k' = k * k_factor, then
//     rerank_kernel: one workgroup per query, the prepared query in registers (a lane holds its one or two pieces of 8
//     components as fp32), one wave per candidate row, four rows in flight per wave -- a gather of k' rows of 2 d bytes,
//     bound by latency and bandwidth; MFMA has no place in it.  That distance is row_score.h's, which annoy_ann.hip
//     shares.  It goes with the candidate's rank in (id, position) order into a 64-bit LDS key, stored complemented;
//     survivor_topk.h's sort_keys_desc over at most 1024 of them, as pq_select_kernel sorts its survivors, gives the answer
//     in (distance, id, position) order, and row_score.h's emit writes it.  No atomics at all.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ivf_ann.h"
#include "../../include/ivfpq_ann.h"
#include "../../include/opq_ann.h"
#include "../../include/refine_ann.h"
#include "ivf_device_rows.h"
#include "faiss_restore.h"
#include "ivf_error.h"  // g_err, fail, ITRY, ABI_CATCH
#include "ivf_kernels.h"
#include "row_score.h"  // load_query, score_rows, emit_sorted

namespace {

// a call into the base: the same status codes, its message is in the base's *_last_error()
#define BCALL(ix, expr)                                                                           \
  do {                                                                                            \
    int rc_ = (expr);                                                                             \
    if (rc_) return fail(rc_, std::string("base index: ") + ((ix)->opq ? opq_last_error() : ivfpq_last_error())); \
  } while (0)
// a call into the inner IVF-PQ index of either base
#define PCALL(expr)                                                                               \
  do {                                                                                            \
    int rc_ = (expr);                                                                             \
    if (rc_) return fail(rc_, std::string("base index: ") + ivfpq_last_error());                  \
  } while (0)

constexpr int MAX_STORE_D = 1024;
constexpr int MAX_CAND = MAX_K;  // k * k_factor: the base's largest k

struct RerankArgs {
  const _Float16 *rows;        // the store, [n][stride]
  const _Float16 *q16;         // prepared queries, [nq][stride]
  const int32_t *pos;          // candidates [nq][width]: add-order positions, best first by the base
  const uint32_t *rank;        // their ranks in (id, position) order
  const int32_t *cnt;          // [nq] candidates per query
  const int64_t *ids_sorted;   // [n] ids by rank
  int64_t n;
  int stride, width, k, metric;
  float *out_dist;             // [nq][k]
  int64_t *out_ids;
  int32_t *out_counts;         // [nq]
};

// One workgroup per query, 256 threads, NP as row_score.h has it.  Wave w scores candidates 4 w .. 4 w + 3, then strides on;
// a candidate's key goes, complemented, to its own slot of the LDS list.
template <int NP>
__global__ __launch_bounds__(256) void rerank_kernel(RerankArgs a) {
  __shared__ unsigned long long keys[MAX_CAND];
  const int t = threadIdx.x, w = t >> 6, q = blockIdx.x;
  const int pieces = a.stride >> 3;
  const int c = min(max(a.cnt[q], 0), a.width);
  uint32_t n2 = 64;
  while (n2 < (uint32_t)c) n2 <<= 1;
  for (uint32_t i = t; i < n2; i += 256) keys[i] = 0;  // the complement of the largest key: sorts last
  float qf[NP][8];
  load_query<NP>(a.q16 + (size_t)q * a.stride, pieces, qf);
  __syncthreads();
  const int32_t *cp = a.pos + (size_t)q * a.width;
  for (int i0 = w * ROWS_IN_FLIGHT; i0 < c; i0 += 4 * ROWS_IN_FLIGHT) {  // (i0 and c are the same for every lane of a wave)
    int64_t pos[ROWS_IN_FLIGHT];
    float dist[ROWS_IN_FLIGHT];
#pragma unroll
    for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
      const int64_t p = i0 + u < c ? (int64_t)cp[i0 + u] : -1;
      pos[u] = p < a.n ? p : -1;
    }
    score_rows<NP>(a.rows, a.stride, pieces, pos, qf, a.metric == IVF_METRIC_L2, dist);
#pragma unroll
    for (int u = 0; u < ROWS_IN_FLIGHT; ++u)
      if ((t & 63) == 0 && pos[u] >= 0)
        keys[i0 + u] = ~(((unsigned long long)f2key(dist[u]) << 32) | a.rank[(size_t)q * a.width + i0 + u]);
  }
  __syncthreads();
  sort_keys_desc(keys, n2);
  // (a key left at 0 among the first c: a candidate outside the store, which cannot happen with the base's own positions)
  emit_sorted(keys, (uint32_t)min(c, a.k), a.k, a.ids_sorted, a.out_dist + (size_t)q * a.k, a.out_ids + (size_t)q * a.k, a.out_counts + q);
}

}  // namespace

struct refine_index {
  int device = 0, metric = 0, d = 0, stride = 0, k_factor = 1;
  ivfpq_index_t *pq = nullptr;  // the base: one of the two
  opq_index_t *opq = nullptr;
  int64_t n = 0;
  Buf rows;                                   // the store
  Buf stage, flat, sumsq;                     // an add's slab: fp32 rows, prepared halves, their sums of squares
  Buf qstage, q16, pos, rank, cnt, o_dist, o_ids, o_cnt;  // a search
  int32_t last_nq = 0, last_width = 0;
  float t_base = 0, t_rerank = 0;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  ~refine_index() {
    if (pq) (void)ivfpq_index_destroy(pq);
    if (opq) (void)opq_index_destroy(opq);
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  ivfpq_index *inner() const { return opq ? opq_internal::inner(opq) : pq; }
};

namespace {

bool k_factor_ok(int32_t k_factor) { return k_factor >= 1 && k_factor <= REFINE_MAX_K_FACTOR; }

int wrap(ivfpq_index_t *pq, opq_index_t *opq, int32_t k_factor, refine_index_t **out) {
  if (!k_factor_ok(k_factor)) return fail(IVF_EINVAL, "k_factor must be in 1..1024");
  if ((!pq && !opq) || !out) return fail(IVF_EINVAL, "null argument");
  std::unique_ptr<refine_index> ix(new refine_index);
  int64_t n = 0;
  int32_t d = 0, metric = 0;
  if (opq) {
    if (int rc = opq_index_info(opq, &n, &d, nullptr, &metric, nullptr, nullptr)) return fail(rc, std::string("base index: ") + opq_last_error());
  } else {
    if (int rc = ivfpq_index_info(pq, &n, &d, &metric, nullptr, nullptr)) return fail(rc, std::string("base index: ") + ivfpq_last_error());
  }
  if (n != 0) return fail(IVF_EINVAL, "the base index holds rows: the store needs every row, wrap an empty base");
  if (d < 1 || d > MAX_STORE_D) return fail(IVF_EINVAL, "dimension must be in 1..1024");
  ix->device = ivfpq_internal::device_of(opq ? opq_internal::inner(opq) : pq);
  ITRY(hipSetDevice(ix->device));
  ix->metric = metric;
  ix->d = d;
  ix->stride = (d + 7) / 8 * 8;
  ix->k_factor = k_factor;
  for (auto &e : ix->ev) ITRY(hipEventCreate(&e));
  ix->pq = pq;  // from here on the handle owns the base
  ix->opq = opq;
  *out = ix.release();
  return IVF_OK;
}

// m prepared rows of d halves (contiguous) -> rows [at, at + m) of a [.][stride] buffer whose padding is zero
int place_rows(const refine_index *ix, const _Float16 *flat, int64_t m, _Float16 *dst, int64_t at) {
  const size_t pitch = (size_t)ix->stride * sizeof(_Float16), width = (size_t)ix->d * sizeof(_Float16);
  ITRY(hipMemsetAsync(dst + (size_t)at * ix->stride, 0, (size_t)m * pitch, 0));
  ITRY(hipMemcpy2DAsync(dst + (size_t)at * ix->stride, pitch, flat, width, width, (size_t)m, hipMemcpyDeviceToDevice, 0));
  return IVF_OK;
}

// m device rows (fp32 [m][d]) -> prepared as the inverted-file indexes prepare a row -> ix->flat
int prepare_rows(refine_index *ix, const float *d_rows, int64_t m) {
  ITRY(ix->flat.reserve((size_t)m * ix->d * sizeof(_Float16)));
  ITRY(ix->sumsq.reserve((size_t)m * sizeof(float)));
  hipLaunchKernelGGL(store_rows_kernel, dim3(blocks_for(m, 4)), dim3(256), 0, 0, d_rows, m, ix->d,
                     ix->metric == IVF_METRIC_COSINE ? 1 : 0, ix->flat.as<_Float16>(), ix->sumsq.as<float>());
  ITRY(hipGetLastError());
  return IVF_OK;
}

int search(refine_index_t *ix, int32_t nq, const float *queries, int32_t k, int32_t nprobe, int32_t k_factor, float *out_dist,
           int64_t *out_ids, int32_t *out_counts) {
  const int width = k * k_factor;
  const int d = ix->d, stride = ix->stride;
  ITRY(hipSetDevice(ix->device));
  ITRY(ix->qstage.reserve((size_t)nq * d * sizeof(float)));
  ITRY(ix->q16.reserve((size_t)nq * stride * sizeof(_Float16)));
  ITRY(ix->pos.reserve((size_t)nq * width * sizeof(int32_t)));
  ITRY(ix->rank.reserve((size_t)nq * width * sizeof(uint32_t)));
  ITRY(ix->cnt.reserve((size_t)nq * sizeof(int32_t)));
  ITRY(ix->o_dist.reserve((size_t)nq * k * sizeof(float)));
  ITRY(ix->o_ids.reserve((size_t)nq * k * sizeof(int64_t)));
  ITRY(ix->o_cnt.reserve((size_t)nq * sizeof(int32_t)));
  ix->last_nq = 0;
  ix->t_base = ix->t_rerank = 0;
  ITRY(hipMemcpy(ix->qstage.p, queries, (size_t)nq * d * sizeof(float), hipMemcpyHostToDevice));
  // the candidates: the base's search at k' = k * k_factor, as positions on the device
  ITRY(hipEventRecord(ix->ev[0], 0));
  if (ix->opq)
    BCALL(ix, opq_internal::search_positions(ix->opq, nq, ix->qstage.as<float>(), width, nprobe, ix->pos.as<int32_t>(),
                                             ix->rank.as<uint32_t>(), ix->cnt.as<int32_t>()));
  else
    BCALL(ix, ivfpq_internal::search_positions(ix->pq, nq, ix->qstage.as<float>(), width, nprobe, ix->pos.as<int32_t>(),
                                               ix->rank.as<uint32_t>(), ix->cnt.as<int32_t>()));
  ITRY(hipEventRecord(ix->ev[1], 0));
  // the re-rank
  if (int rc = prepare_rows(ix, ix->qstage.as<float>(), nq)) return rc;
  if (int rc = place_rows(ix, ix->flat.as<_Float16>(), nq, ix->q16.as<_Float16>(), 0)) return rc;
  RerankArgs a;
  a.rows = ix->rows.as<_Float16>();
  a.q16 = ix->q16.as<_Float16>();
  a.pos = ix->pos.as<int32_t>();
  a.rank = ix->rank.as<uint32_t>();
  a.cnt = ix->cnt.as<int32_t>();
  a.ids_sorted = ivfpq_internal::device_ids_sorted(ix->inner());
  a.n = ix->n;
  a.stride = stride;
  a.width = width;
  a.k = k;
  a.metric = ix->metric;
  a.out_dist = ix->o_dist.as<float>();
  a.out_ids = ix->o_ids.as<int64_t>();
  a.out_counts = ix->o_cnt.as<int32_t>();
  if (stride <= 512) hipLaunchKernelGGL(rerank_kernel<1>, dim3(nq), dim3(256), 0, 0, a);
  else hipLaunchKernelGGL(rerank_kernel<2>, dim3(nq), dim3(256), 0, 0, a);
  ITRY(hipGetLastError());
  ITRY(hipEventRecord(ix->ev[2], 0));
  ITRY(hipMemcpyAsync(out_dist, ix->o_dist.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, 0));
  ITRY(hipMemcpyAsync(out_ids, ix->o_ids.p, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, 0));
  ITRY(hipMemcpyAsync(out_counts, ix->o_cnt.p, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, 0));
  ITRY(hipStreamSynchronize(0));
  (void)hipEventElapsedTime(&ix->t_base, ix->ev[0], ix->ev[1]);
  (void)hipEventElapsedTime(&ix->t_rerank, ix->ev[1], ix->ev[2]);
  ix->last_nq = nq;
  ix->last_width = width;
  return IVF_OK;
}

// everything a search refuses before it makes a device call
int check_search(const refine_index_t *ix, int32_t nq, const float *queries, int32_t k, int32_t nprobe, int32_t k_factor,
                 const float *out_dist, const int64_t *out_ids, const int32_t *out_counts) {
  if (!ix || !queries || !out_dist || !out_ids || !out_counts) return fail(IVF_EINVAL, "null argument");
  if (nq < 1) return fail(IVF_EINVAL, "nq must be positive");
  if (k < 1 || k > MAX_K) return fail(IVF_EINVAL, "k must be in 1..1024");
  if (!k_factor_ok(k_factor)) return fail(IVF_EINVAL, "k_factor must be in 1..1024");
  if ((int64_t)k * k_factor > MAX_CAND)
    return fail(IVF_EINVAL, "k * k_factor = " + std::to_string((int64_t)k * k_factor) + " exceeds 1024, the most the base index answers");
  if (nprobe < 1 || nprobe > MAX_NPROBE) return fail(IVF_EINVAL, "nprobe must be in 1..1024");
  return IVF_OK;
}

}  // namespace

extern "C" {

const char *refine_last_error(void) { return g_err.c_str(); }

int refine_index_wrap_ivfpq(ivfpq_index_t *base, int32_t k_factor, refine_index_t **out) try {
  return wrap(base, nullptr, k_factor, out);
} ABI_CATCH

int refine_index_wrap_opq(opq_index_t *base, int32_t k_factor, refine_index_t **out) try {
  return wrap(nullptr, base, k_factor, out);
} ABI_CATCH

int refine_index_add(refine_index_t *ix, int64_t n, const float *vectors, const int64_t *ids) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (n < 0) return fail(IVF_EINVAL, "n must not be negative");
  if (n > 0 && !vectors) return fail(IVF_EINVAL, "null vectors");
  ITRY(hipSetDevice(ix->device));
  if (n == 0) {  // the ids rule still speaks, as in the base
    BCALL(ix, ix->opq ? opq_index_add(ix->opq, 0, vectors, ids) : ivfpq_index_add(ix->pq, 0, vectors, ids));
    return IVF_OK;
  }
  const int d = ix->d, stride = ix->stride;
  // the base refuses here what it refuses (the ids rule, the row count) and makes room; it is unchanged until add_end
  PCALL(ivfpq_internal::add_begin(ix->inner(), n, ids != nullptr));
  const int64_t n_old = ix->n, total = n_old + n;
  ITRY(ix->rows.grow_keep((size_t)n_old * stride * sizeof(_Float16), (size_t)total * stride * sizeof(_Float16)));
  const int64_t slab = ix->opq ? opq_internal::slab_rows(ix->opq) : ivfpq_internal::slab_rows(d);
  ITRY(ix->stage.reserve((size_t)std::min(slab, n) * d * sizeof(float)));
  for (int64_t r0 = 0; r0 < n; r0 += slab) {
    const int64_t m = std::min(slab, n - r0);
    ITRY(hipMemcpy(ix->stage.p, vectors + r0 * d, (size_t)m * d * sizeof(float), hipMemcpyHostToDevice));
    // the store first (behind the rows that count), then the base's slab
    if (int rc = prepare_rows(ix, ix->stage.as<float>(), m)) return rc;
    if (int rc = place_rows(ix, ix->flat.as<_Float16>(), m, ix->rows.as<_Float16>(), n_old + r0)) return rc;
    ITRY(hipDeviceSynchronize());
    if (ix->opq) BCALL(ix, opq_internal::add_slab(ix->opq, r0, m, ix->stage.as<float>()));
    else BCALL(ix, ivfpq_internal::add_slab(ix->pq, r0, m, ix->stage.as<float>()));
  }
  PCALL(ivfpq_internal::add_end(ix->inner(), n, ids));
  ix->n = total;
  return IVF_OK;
} ABI_CATCH

int refine_search_with_k_factor(refine_index_t *ix, int32_t nq, const float *queries, int32_t k, int32_t nprobe, int32_t k_factor,
                                float *out_dist, int64_t *out_ids, int32_t *out_counts) try {
  // (the numbers are refused before the handle is looked at)
  if (int rc = check_search(ix, nq, queries, k, nprobe, k_factor, out_dist, out_ids, out_counts)) return rc;
  return search(ix, nq, queries, k, nprobe, k_factor, out_dist, out_ids, out_counts);
} ABI_CATCH

int refine_search(refine_index_t *ix, int32_t nq, const float *queries, int32_t k, int32_t nprobe, float *out_dist, int64_t *out_ids,
                  int32_t *out_counts) try {
  if (!ix) return fail(IVF_EINVAL, "null argument");
  return refine_search_with_k_factor(ix, nq, queries, k, nprobe, ix->k_factor, out_dist, out_ids, out_counts);
} ABI_CATCH

int refine_index_set_k_factor(refine_index_t *ix, int32_t k_factor) try {
  if (!k_factor_ok(k_factor)) return fail(IVF_EINVAL, "k_factor must be in 1..1024");
  if (!ix) return fail(IVF_EINVAL, "null index");
  ix->k_factor = k_factor;
  return IVF_OK;
} ABI_CATCH

int refine_index_info(const refine_index_t *ix, int64_t *n, int32_t *d, int32_t *metric, int32_t *k_factor, int32_t *base_kind) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (n) *n = ix->n;
  if (d) *d = ix->d;
  if (metric) *metric = ix->metric;
  if (k_factor) *k_factor = ix->k_factor;
  if (base_kind) *base_kind = ix->opq ? REFINE_BASE_OPQ : REFINE_BASE_IVFPQ;
  return IVF_OK;
} ABI_CATCH

int refine_index_base(const refine_index_t *ix, int32_t *base_kind, void **base) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (base_kind) *base_kind = ix->opq ? REFINE_BASE_OPQ : REFINE_BASE_IVFPQ;
  if (base) *base = ix->opq ? (void *)ix->opq : (void *)ix->pq;
  return IVF_OK;
} ABI_CATCH

int refine_last_candidates(const refine_index_t *ix, int32_t *nq, int32_t *width, int32_t *out_positions, int32_t *out_counts) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (nq) *nq = ix->last_nq;
  if (width) *width = ix->last_nq > 0 ? ix->last_width : 0;
  if (ix->last_nq > 0 && (out_positions || out_counts)) {
    ITRY(hipSetDevice(ix->device));
    if (out_positions)
      ITRY(hipMemcpy(out_positions, ix->pos.p, (size_t)ix->last_nq * ix->last_width * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (out_counts) ITRY(hipMemcpy(out_counts, ix->cnt.p, (size_t)ix->last_nq * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return IVF_OK;
} ABI_CATCH

int refine_index_get_rows(const refine_index_t *ix, int64_t row0, int64_t m, uint16_t *out) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (row0 < 0 || m < 0 || row0 > ix->n || m > ix->n - row0) return fail(IVF_EINVAL, "rows outside the index");
  if (m == 0) return IVF_OK;
  if (!out) return fail(IVF_EINVAL, "null argument");
  ITRY(hipSetDevice(ix->device));
  const size_t pitch = (size_t)ix->stride * sizeof(_Float16), width = (size_t)ix->d * sizeof(_Float16);
  ITRY(hipMemcpy2D(out, width, ix->rows.as<_Float16>() + (size_t)row0 * ix->stride, pitch, width, (size_t)m, hipMemcpyDeviceToHost));
  return IVF_OK;
} ABI_CATCH

int refine_last_stats(const refine_index_t *ix, float *base_ms, float *rerank_ms) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (base_ms) *base_ms = ix->t_base;
  if (rerank_ms) *rerank_ms = ix->t_rerank;
  return IVF_OK;
} ABI_CATCH

int refine_index_destroy(refine_index_t *ix) try {
  delete ix;
  return IVF_OK;
} ABI_CATCH

}  // extern "C"
