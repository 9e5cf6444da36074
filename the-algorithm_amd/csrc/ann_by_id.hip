// ann_by_id.hip -- the device-resident embedding store and the by-id queries of include/ann_by_id.h.
//
// A by-id query is the plain search with another first half:
//   1 resolve   the seed ids are uploaded (8 bytes each), each looks itself up in the producer's (key, position) table sorted by
//               key, and an exclusive scan of the found flags gives every found seed its compact query slot
//   2 gather    one wave per seed: the producer's row goes through LDS (16-byte loads) and is prepared with the arithmetic of
//               the index's own query preparation (hnsw_prep_rows / prep_rows_kernel: fp64 sum of squares, lane l summing
//               elements l, l + 64, ... in that order, then the xor tree; one sqrt; fp32 divide; rounding to fp16) straight into
//               the index's prepared-query buffer at the slot.  An exact-mode brute-force index also gets the fp32 row in q_in
//   3 search    the index's own second half (ann_by_id_internal.h), unchanged
//   4 flatten   an exclusive scan of the per-seed counts, then one wave per seed writes its (seed, id, distance) triples at its
//               offset; out_total triples and the counts are all that is copied back
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ann_by_id.h"
#include "ann_by_id_internal.h"
#include "by_id_core.h"  // resolve, flatten, the scratch; Buf, g_err, fail, BTRY
#define ABI_CATCH catch (...) { return abi_guard::caught(fail, ANN_BY_ID_ENOMEM, ANN_BY_ID_EINTERNAL); }

namespace {

constexpr int MAX_D = 512;

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

// ---- kernels ---------------------------------------------------------------------------------------------------------

__global__ void by_id_iota_kernel(int64_t *__restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = i;
}

// sorted keys: the first index whose key repeats its predecessor's is left in *bad (which starts at INT32_MAX)
__global__ void by_id_repeat_kernel(const int64_t *__restrict__ keys, int64_t n, int32_t *__restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 1 || i >= n) return;
  if (keys[i - 1] == keys[i]) atomicMin(bad, (int32_t)i);
}

// (the resolve, seed-count and flatten kernels are by_id_core.h's)

// Where the producer's rows come from.
constexpr int SRC_F32 = 0;    // store: fp32 [n][d]
constexpr int SRC_HNSW = 1;   // hnsw index: fp16 [n][dpad]
constexpr int SRC_FRAG = 2;   // brute-force index: fp16 MFMA fragments (dense_ann.hip prep_rows_kernel)
// Where the prepared query goes.
constexpr int DST_HNSW = 0;   // fp16 [slot][dpad]
constexpr int DST_FRAG = 1;   // fragments + qsumsq[slot] (+ q_in[slot][d] fp32 in exact mode)

struct GatherArgs {
  const void *src;
  int64_t src_stride;            // SRC_F32: d; SRC_HNSW: dpad; SRC_FRAG: S
  const int64_t *pos;            // [n_seeds] row of the seed, -1 absent
  const int32_t *slot;           // [n_seeds] compact slot of a found seed
  int64_t n_seeds;
  int slot0, slot_n;             // the slots this launch prepares: [slot0, slot0 + slot_n), written at slot - slot0
  int d, dst_stride;             // DST_HNSW: dpad; DST_FRAG: S
  int normalise;
  _Float16 *dst;
  float *qsumsq, *q_in;          // DST_FRAG (q_in may be NULL)
};

// One wave per seed, four per workgroup.  The row is staged in LDS as fp32 so that the loads can be 16 bytes wide while every
// lane still sums the elements the plain preparation gives it, in its order.
template <int SRC, int DST>
__global__ __launch_bounds__(256) void by_id_gather_prep_kernel(GatherArgs a) {
  __shared__ __attribute__((aligned(16))) float rows[4][MAX_D];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + w;
  int64_t row = -1;
  int slot = 0;
  if (i < a.n_seeds) {
    row = a.pos[i];
    slot = a.slot[i] - a.slot0;
  }
  const bool active = row >= 0 && slot >= 0 && slot < a.slot_n;
  float *x = rows[w];
  const int d = a.d;
  if (active) {
    if (SRC == SRC_F32) {
      const float *s = (const float *)a.src + row * a.src_stride;
      if ((d & 3) == 0) {  // rows start on 16 bytes: hipMalloc's alignment plus a multiple of 16 bytes per row
        const float4 *s4 = (const float4 *)s;
        for (int c = lane; c < d / 4; c += 64) ((float4 *)x)[c] = s4[c];
      } else {
        for (int k = lane; k < d; k += 64) x[k] = s[k];
      }
    } else if (SRC == SRC_HNSW) {  // dpad is a multiple of 64 halves: whole 16-byte chunks (the padding is zeros, unread below)
      const half8 *s8 = (const half8 *)((const _Float16 *)a.src + row * a.src_stride);
      for (int c = lane; c * 8 < d; c += 64) {
        const half8 v = s8[c];
        for (int j = 0; j < 8; ++j)
          if (c * 8 + j < d) x[c * 8 + j] = (float)v[j];
      }
    } else {  // element k of row r of block g: fragment ((g * S + k / 16) * 64 + ((k / 8) & 1) * 32 + r) * 8 + k % 8
      const int64_t g = row >> 5, S = a.src_stride;
      const int r = (int)(row & 31);
      const half8 *f8 = (const half8 *)a.src;
      for (int c = lane; c * 8 < d; c += 64) {
        const half8 v = f8[(g * S + (c >> 1)) * 64 + (c & 1) * 32 + r];
        for (int j = 0; j < 8; ++j)
          if (c * 8 + j < d) x[c * 8 + j] = (float)v[j];
      }
    }
  }
  __syncthreads();
  if (!active) return;
  // from here on: hnsw_prep_rows (DST_HNSW) / prep_rows_kernel (DST_FRAG) with x in LDS
  float norm = 1.0f;
  if (a.normalise) {
    double ss = 0;
    for (int k = lane; k < d; k += 64) ss += (double)x[k] * (double)x[k];
    for (int o = 32; o; o >>= 1) ss += __shfl_xor(ss, o, 64);
    norm = (float)sqrt(ss);
    if (!(norm > 0.0f)) norm = 1.0f;
  }
  if (DST == DST_HNSW) {
    const int dpad = a.dst_stride;
    _Float16 *y = a.dst + (int64_t)slot * dpad;
    for (int k = lane; k < dpad; k += 64) y[k] = (_Float16)(k < d ? x[k] / norm : 0.0f);
  } else {
    const int S = a.dst_stride;
    const int64_t g = slot >> 5;
    const int r = slot & 31;
    double ss16 = 0;
    for (int k = lane; k < S * 16; k += 64) {
      float v = k < d ? x[k] / norm : 0.0f;
      _Float16 hv = (_Float16)v;
      float back = (float)hv;
      ss16 += (double)back * (double)back;
      int s = k >> 4, h = (k >> 3) & 1, j = k & 7;
      a.dst[(((g * S + s) * 64) + h * 32 + r) * 8 + j] = hv;
    }
    for (int o = 32; o; o >>= 1) ss16 += __shfl_xor(ss16, o, 64);
    if (lane == 0) a.qsumsq[slot] = (float)ss16;
    if (a.q_in) {
      float *q = a.q_in + (int64_t)slot * d;
      for (int k = lane; k < d; k += 64) q[k] = x[k];
    }
  }
}

// ann_store_get: rows of the resolved keys (zeros for an absent one) and the found bytes
__global__ void by_id_get_kernel(const float *__restrict__ rows, int d, const int64_t *__restrict__ pos, int64_t n,
                                 float *__restrict__ out, uint8_t *__restrict__ found) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= n) return;
  const int64_t p = pos[i];
  for (int k = lane; k < d; k += 64) out[i * d + k] = p >= 0 ? rows[p * d + k] : 0.0f;
  if (lane == 0) found[i] = p >= 0 ? 1 : 0;
}

// (key, position) sorted by key from n keys on the device
int sort_key_positions(const int64_t *d_keys, int64_t n, Buf &keys, Buf &pos) {
  size_t tb = 0;
  BTRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const int64_t *)nullptr, (int64_t *)nullptr, (const int64_t *)nullptr,
                                          (int64_t *)nullptr, (int)n, 0, 64, (hipStream_t)0));
  Buf tmp, iota;
  BTRY(tmp.reserve(tb));
  BTRY(iota.reserve((size_t)n * 8));
  BTRY(keys.reserve((size_t)n * 8));
  BTRY(pos.reserve((size_t)n * 8));
  hipLaunchKernelGGL(by_id_iota_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, iota.as<int64_t>(), n);
  BTRY(hipGetLastError());
  BTRY(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, d_keys, keys.as<int64_t>(), iota.as<int64_t>(), pos.as<int64_t>(), (int)n, 0, 64,
                                          (hipStream_t)0));
  BTRY(hipDeviceSynchronize());  // (before tmp and iota are freed)
  return ANN_BY_ID_OK;
}

}  // namespace

struct ann_store {
  int device = 0, d = 0;
  int64_t n = 0;
  Buf rows, keys, pos;  // fp32 [n][d]; (key, position) sorted by key
};

namespace {

// The producer of a call: the store's table and rows, or the index's own.
struct Producer : KeyTable {
  const void *rows = nullptr;
  int64_t stride = 0;
  int src = SRC_F32;
};

int check_store(const ann_store *store, int device, int d) {
  if (!store) return ANN_BY_ID_OK;
  if (store->d != d)
    return fail(ANN_BY_ID_EINVAL, "the store holds rows of dimension " + std::to_string(store->d) + ", the index of " + std::to_string(d));
  if (store->device != device)
    return fail(ANN_BY_ID_EINVAL, "the store is on device " + std::to_string(store->device) + ", the index on " + std::to_string(device));
  return ANN_BY_ID_OK;
}

template <int DST>
int launch_gather(const Producer &p, const GatherArgs &a) {
  const dim3 grid((unsigned)((a.n_seeds + 3) / 4)), block(256);
  if (p.src == SRC_F32) hipLaunchKernelGGL((by_id_gather_prep_kernel<SRC_F32, DST>), grid, block, 0, 0, a);
  else if (p.src == SRC_HNSW) hipLaunchKernelGGL((by_id_gather_prep_kernel<SRC_HNSW, DST>), grid, block, 0, 0, a);
  else hipLaunchKernelGGL((by_id_gather_prep_kernel<SRC_FRAG, DST>), grid, block, 0, 0, a);
  BTRY(hipGetLastError());
  return ANN_BY_ID_OK;
}

}  // namespace

// the store as faiss_by_id.hip sees it (ann_by_id_internal.h)
int ann_by_id::store_view(const ann_store *store, StoreView *out) {
  out->device = store->device;
  out->d = store->d;
  out->n = store->n;
  out->keys = store->keys.as<int64_t>();
  out->kpos = store->pos.as<int64_t>();
  out->rows = store->rows.as<float>();
  return ANN_BY_ID_OK;
}

extern "C" {

const char *ann_by_id_last_error(void) { return g_err.c_str(); }

int ann_store_build(int32_t device, int64_t n, int32_t d, const int64_t *keys, const float *vectors, ann_store_t **out) try {
  if (!out) return fail(ANN_BY_ID_EINVAL, "NULL argument");
  *out = nullptr;
  if (d < 1 || d > MAX_D) return fail(ANN_BY_ID_EINVAL, "dimension must be in 1..512");
  if (n < 0 || n >= (int64_t)0x7fffffff) return fail(ANN_BY_ID_EINVAL, "row count out of range");
  if (n > 0 && (!keys || !vectors)) return fail(ANN_BY_ID_EINVAL, "NULL argument");
  BTRY(hipSetDevice(device));
  std::unique_ptr<ann_store> s(new ann_store);
  s->device = device;
  s->d = d;
  s->n = n;
  if (n > 0) {
    Buf in, bad;
    BTRY(in.reserve((size_t)n * 8));
    BTRY(bad.reserve(4));
    BTRY(hipMemcpy(in.p, keys, (size_t)n * 8, hipMemcpyHostToDevice));
    if (int rc = sort_key_positions(in.as<int64_t>(), n, s->keys, s->pos)) return rc;
    BTRY(hipMemsetAsync(bad.p, 0x7f, 4, 0));
    hipLaunchKernelGGL(by_id_repeat_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, s->keys.as<int64_t>(), n, bad.as<int32_t>());
    BTRY(hipGetLastError());
    int32_t b = 0;
    BTRY(hipMemcpy(&b, bad.p, 4, hipMemcpyDeviceToHost));
    if (b >= 0 && b < n) {
      int64_t key = 0;
      BTRY(hipMemcpy(&key, s->keys.as<int64_t>() + b, 8, hipMemcpyDeviceToHost));
      return fail(ANN_BY_ID_EINVAL, "duplicate key " + std::to_string(key) + ": it appears twice in the store's keys");
    }
    BTRY(s->rows.reserve((size_t)n * d * 4));
    BTRY(hipMemcpy(s->rows.p, vectors, (size_t)n * d * 4, hipMemcpyHostToDevice));
  }
  *out = s.release();
  return ANN_BY_ID_OK;
} ABI_CATCH

int ann_store_info(const ann_store_t *store, int64_t *n, int32_t *d) try {
  if (!store) return fail(ANN_BY_ID_EINVAL, "NULL store");
  if (n) *n = store->n;
  if (d) *d = store->d;
  return ANN_BY_ID_OK;
} ABI_CATCH

int ann_store_get(const ann_store_t *store, int64_t n, const int64_t *keys, float *out_vectors, uint8_t *out_found) try {
  if (!store) return fail(ANN_BY_ID_EINVAL, "NULL store");
  if (n < 0 || n >= (int64_t)0x7fffffff) return fail(ANN_BY_ID_EINVAL, "key count out of range");
  if (n == 0) return ANN_BY_ID_OK;
  if (!keys || !out_vectors || !out_found) return fail(ANN_BY_ID_EINVAL, "NULL argument");
  BTRY(hipSetDevice(store->device));
  const int d = store->d;
  Buf q, pos, flag, rows, found;  // (a store is shared between threads: nothing of a call is kept on it)
  BTRY(q.reserve((size_t)n * 8));
  BTRY(pos.reserve((size_t)n * 8));
  BTRY(flag.reserve((size_t)n * 4));
  BTRY(rows.reserve((size_t)n * d * 4));
  BTRY(found.reserve((size_t)n));
  BTRY(hipMemcpy(q.p, keys, (size_t)n * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(by_id_resolve_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, store->keys.as<int64_t>(),
                     store->pos.as<int64_t>(), store->n, 0, q.as<int64_t>(), n, pos.as<int64_t>(), flag.as<int32_t>());
  BTRY(hipGetLastError());
  hipLaunchKernelGGL(by_id_get_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, 0, store->rows.as<float>(), d, pos.as<int64_t>(), n,
                     rows.as<float>(), found.as<uint8_t>());
  BTRY(hipGetLastError());
  BTRY(hipMemcpy(out_vectors, rows.p, (size_t)n * d * 4, hipMemcpyDeviceToHost));
  BTRY(hipMemcpy(out_found, found.p, (size_t)n, hipMemcpyDeviceToHost));
  return ANN_BY_ID_OK;
} ABI_CATCH

int ann_store_destroy(ann_store_t *store) try {
  delete store;
  return ANN_BY_ID_OK;
} ABI_CATCH

int hnsw_batch_query_by_id(hnsw_index_t *index, const ann_store_t *store, int32_t n_seeds, const int64_t *seeds, int32_t k, int32_t ef,
                           int64_t *out_seed, int64_t *out_id, float *out_dist, int64_t cap, int64_t *out_total,
                           int32_t *out_counts) try {
  if (k < 1 || ef < 1) return fail(HNSW_EINVAL, "k and ef must be positive");
  if (int rc = check_common(index, n_seeds, seeds, out_seed, out_id, out_dist, cap, out_total, out_counts)) return rc;
  ann_by_id::HnswTarget t;
  if (int rc = ann_by_id::hnsw_open(index, n_seeds, k, ef, store == nullptr, &t)) return fail(rc, hnsw_last_error());
  if (int rc = check_store(store, t.device, t.d)) return rc;
  *out_total = 0;
  Scratch *s = nullptr;
  if (int rc = get_scratch(ann_by_id::hnsw_scratch(index), &s)) return rc;
  if (n_seeds == 0) {
    s->found = s->absent = s->h2d = s->d2h = s->d2h_result = 0;
    return ANN_BY_ID_OK;
  }
  Producer p;
  if (store) {
    p.keys = store->keys.as<int64_t>();
    p.kpos = store->pos.as<int64_t>();
    p.nt = store->n;
    p.rows = store->rows.p;
    p.stride = store->d;
    p.src = SRC_F32;
  } else {
    p.keys = t.kp_keys;
    p.kpos = t.kp_pos;
    p.nt = t.kp_keys ? t.kp_n : t.n;
    p.positional = t.kp_keys == nullptr;
    p.rows = t.x;
    p.stride = t.dpad;
    p.src = SRC_HNSW;
  }
  if (int rc = resolve(s, p, n_seeds, seeds)) return rc;
  if (int rc = cap_check(s, k, cap)) return rc;
  hipStream_t st = 0;
  const int32_t nq = (int32_t)s->found;
  ann_by_id::DeviceResult r;
  if (nq > 0 && !t.empty) {
    GatherArgs a;
    a.src = p.rows;
    a.src_stride = p.stride;
    a.pos = s->pos.as<int64_t>();
    a.slot = s->slot.as<int32_t>();
    a.n_seeds = n_seeds;
    a.slot0 = 0;
    a.slot_n = nq;
    a.d = t.d;
    a.dst_stride = t.dpad;
    a.normalise = t.metric == HNSW_METRIC_COSINE ? 1 : 0;
    a.dst = t.q;
    a.qsumsq = a.q_in = nullptr;
    if (int rc = launch_gather<DST_HNSW>(p, a)) return rc;
    BTRY(hipEventRecord(s->ev[1], st));
    if (int rc = ann_by_id::hnsw_search_prepared(index, nq, k, ef, &r)) return fail(rc, hnsw_last_error());
    s->h2d += r.h2d_bytes;
    s->d2h += r.d2h_bytes;
  } else {
    BTRY(hipEventRecord(s->ev[1], st));
  }
  if (int rc = flatten(s, n_seeds, k, r.dist, r.ids, r.counts, out_seed, out_id, out_dist, out_total, out_counts)) return rc;
  (void)hipEventElapsedTime(&s->t_gather, s->ev[0], s->ev[1]);
  (void)hipEventElapsedTime(&s->t_search, s->ev[1], s->ev[2]);
  return ANN_BY_ID_OK;
} ABI_CATCH

int dann_batch_query_by_id(dann_index_t *index, const ann_store_t *store, int32_t n_seeds, const int64_t *seeds, int32_t k,
                           int64_t *out_seed, int64_t *out_id, float *out_dist, int64_t cap, int64_t *out_total,
                           int32_t *out_counts) try {
  if (k < 1 || k > 1024) return fail(DANN_EINVAL, "k must be in 1..1024");
  if (int rc = check_common(index, n_seeds, seeds, out_seed, out_id, out_dist, cap, out_total, out_counts)) return rc;
  ann_by_id::DannTarget t;
  if (int rc = ann_by_id::dann_open(index, k, store == nullptr, &t)) return fail(rc, dann_last_error());
  if (int rc = check_store(store, t.device, t.d)) return rc;
  *out_total = 0;
  Scratch *s = nullptr;
  if (int rc = get_scratch(ann_by_id::dann_scratch(index), &s)) return rc;
  if (n_seeds == 0) {
    s->found = s->absent = s->h2d = s->d2h = s->d2h_result = 0;
    return ANN_BY_ID_OK;
  }
  Producer p;
  if (store) {
    p.keys = store->keys.as<int64_t>();
    p.kpos = store->pos.as<int64_t>();
    p.nt = store->n;
    p.rows = store->rows.p;
    p.stride = store->d;
    p.src = SRC_F32;
  } else {
    p.keys = t.kp_keys;
    p.kpos = t.kp_pos;
    p.nt = t.kp_keys ? t.kp_n : t.n;
    p.positional = t.kp_keys == nullptr;
    p.rows = t.xf;
    p.stride = t.S;
    p.src = SRC_FRAG;
  }
  if (int rc = resolve(s, p, n_seeds, seeds)) return rc;
  if (int rc = cap_check(s, k, cap)) return rc;
  hipStream_t st = 0;
  const int32_t nq = (int32_t)s->found;
  BTRY(s->r_dist.reserve((size_t)nq * k * 4));
  BTRY(s->r_ids.reserve((size_t)nq * k * 8));
  BTRY(s->r_cnt.reserve((size_t)std::max(nq, 1) * 4));
  float t_gather = 0, t_search = 0;
  // chunks of DANN_CHUNK queries, as dann_search runs them (the GEMM keeps one threshold per query in LDS)
  for (int32_t q0 = 0; q0 < nq; q0 += ann_by_id::DANN_CHUNK) {
    const int32_t m = std::min<int32_t>(ann_by_id::DANN_CHUNK, nq - q0);
    if (q0 > 0) BTRY(hipEventRecord(s->ev[0], st));
    ann_by_id::DannChunk c;
    if (int rc = ann_by_id::dann_chunk_open(index, m, k, &c)) return fail(rc, dann_last_error());
    GatherArgs a;
    a.src = p.rows;
    a.src_stride = p.stride;
    a.pos = s->pos.as<int64_t>();
    a.slot = s->slot.as<int32_t>();
    a.n_seeds = n_seeds;
    a.slot0 = q0;
    a.slot_n = m;
    a.d = t.d;
    a.dst_stride = t.S;
    a.normalise = t.metric == DANN_METRIC_COSINE ? 1 : 0;
    a.dst = c.qf;
    a.qsumsq = c.qsumsq;
    a.q_in = t.exact ? c.q_in : nullptr;
    if (int rc = launch_gather<DST_FRAG>(p, a)) return rc;
    BTRY(hipEventRecord(s->ev[1], st));
    int64_t d2h = 0;
    if (int rc = ann_by_id::dann_chunk_search_prepared(index, m, k, s->r_dist.as<float>() + (size_t)q0 * k, s->r_ids.as<int64_t>() + (size_t)q0 * k,
                                                       s->r_cnt.as<int32_t>() + q0, &d2h))
      return fail(rc, dann_last_error());
    s->d2h += d2h;
    BTRY(hipEventRecord(s->ev[2], st));
    BTRY(hipEventSynchronize(s->ev[2]));
    float a_ms = 0, b_ms = 0;
    (void)hipEventElapsedTime(&a_ms, s->ev[0], s->ev[1]);
    (void)hipEventElapsedTime(&b_ms, s->ev[1], s->ev[2]);
    t_gather += a_ms;
    t_search += b_ms;
  }
  if (nq == 0) {
    BTRY(hipEventRecord(s->ev[1], st));
    BTRY(hipEventSynchronize(s->ev[1]));
    (void)hipEventElapsedTime(&t_gather, s->ev[0], s->ev[1]);
  }
  if (int rc = flatten(s, n_seeds, k, s->r_dist.as<float>(), s->r_ids.as<int64_t>(), nq > 0 ? s->r_cnt.as<int32_t>() : nullptr, out_seed,
                       out_id, out_dist, out_total, out_counts))
    return rc;
  s->t_gather = t_gather;
  s->t_search = t_search;
  return ANN_BY_ID_OK;
} ABI_CATCH

int ann_by_id_last_stats(const hnsw_index_t *hnsw, const dann_index_t *dann, int64_t *found, int64_t *absent, int64_t *h2d_bytes,
                         int64_t *d2h_bytes, int64_t *d2h_result_bytes, float *resolve_gather_ms, float *search_ms,
                         float *flatten_ms) try {
  if ((hnsw == nullptr) == (dann == nullptr)) return fail(ANN_BY_ID_EINVAL, "exactly one of the two indexes must be given");
  const std::shared_ptr<void> &slot = hnsw ? ann_by_id::hnsw_scratch(const_cast<hnsw_index_t *>(hnsw))
                                           : ann_by_id::dann_scratch(const_cast<dann_index_t *>(dann));
  static const Scratch none;
  const Scratch *s = slot ? static_cast<const Scratch *>(slot.get()) : &none;
  if (found) *found = s->found;
  if (absent) *absent = s->absent;
  if (h2d_bytes) *h2d_bytes = s->h2d;
  if (d2h_bytes) *d2h_bytes = s->d2h;
  if (d2h_result_bytes) *d2h_result_bytes = s->d2h_result;
  if (resolve_gather_ms) *resolve_gather_ms = s->t_gather;
  if (search_ms) *search_ms = s->t_search;
  if (flatten_ms) *flatten_ms = s->t_flatten;
  return ANN_BY_ID_OK;
} ABI_CATCH

}  // extern "C"
