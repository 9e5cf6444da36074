// shard_set.hip -- a set of inverted-file indexes served as one index (include/shard_set.h) for gfx950.
//
// What it replaces: the reference's sharded Faiss serving (ann/src/main/scala/com/twitter/ann/faiss/HourlyShardedIndex.scala:
// 66-93: the newest hourly directories as one IndexShards(dimension, false, false) behind the QueryableIndexAdapter), which
// this project served by a host loop: every shard's own search from host memory, then dann_compose_shards' std::sort per
// query.
//
// Shape of the computation.
//   * A search takes its queries DANN_CHUNK at a time.  A chunk is uploaded once.  Every member searches it where it lies
//     (ivf_device_rows.h: search_device_out) and leaves its answer in the set's shard buffer A; nothing but the members'
//     control words crosses the bus.  After each member one fold_kernel launch merges A into the running answer R, kept in
//     two buffers that swap roles; after the last member R is downloaded once.
//   * fold_kernel.  Per query the union of R[q] (<= k entries) and A[q] (<= k_in entries) is sorted by (distance, id) and
//     the best k are written.  A member's run is NOT sorted by (distance, id) -- the select kernels order by (score, id
//     rank) and distinct scores can round to one distance -- so the union is sorted, not merged: a bitonic network in LDS
//     over (distance key, id), the entry's own distance bits carried along.  The key is the order-preserving integer image
//     of the float with -0.0 made +0.0 first, so the order is the host comparator's (a.d < b.d || (a.d == b.d && a.id <
//     b.id)) for every distance that is not NaN.  The network is sized to the next power of two >= the entries the
//     workgroup's queries really hold, not to k + k_in.  For small k a workgroup takes several queries side by side: a
//     bitonic network whose every merge starts with a mirrored step sorts all its aligned segments ascending at once.
//   * A by-id search (include/faiss_by_id.h, through shardset_internal::search_store_out) differs in the two ends of a chunk
//     alone: gather_rows_kernel copies the chunk's rows out of the device-resident store into the query buffer instead of the
//     upload, and the running answer is copied device to device into the caller's buffers instead of the download.
//   * shardset_compose is the same kernel over host runs: the runs of one shard are uploaded and folded, shard by shard.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/faiss_files.h"
#include "../../include/ivf_ann.h"
#include "../../include/ivfpq_ann.h"
#include "../../include/opq_ann.h"
#include "../../include/shard_set.h"
#include "ann_by_id_internal.h"  // DANN_CHUNK
#include "device_buf.h"
#include "ivf_device_rows.h"
#include "ivf_error.h"  // g_err, fail, ITRY, ABI_CATCH

namespace {

constexpr int MAX_K = 1024;
constexpr int MAX_NPROBE = 1024;
constexpr int CHUNK = ann_by_id::DANN_CHUNK;
constexpr int FOLD_THREADS = 256;
constexpr int FOLD_QPW = 16;             // queries a workgroup takes at most
constexpr uint32_t FOLD_ENTRIES = 512;   // entries a workgroup of several queries sorts: one comparator per thread and step

struct FoldArgs {
  // the running answer: [nq][k] and [nq]; r_cnt == NULL: there is none yet
  const float *r_dist;
  const int64_t *r_ids;
  const int32_t *r_cnt;
  // a member's answer: [nq][k_a] and [nq]
  const float *a_dist;
  const int64_t *a_ids;
  const int32_t *a_cnt;
  // the next running answer: [nq][k] and [nq]
  float *o_dist;
  int64_t *o_ids;
  int32_t *o_cnt;
  int32_t nq, k, k_a;
  uint32_t seg;  // a power of two >= max(2, k + k_a): the LDS entries of one query
  uint32_t qpw;  // queries per workgroup, a power of two; the workgroup's dynamic LDS is fold_lds_bytes(qpw * seg)
};

inline uint32_t pow2_at_least(uint32_t n) {
  uint32_t p = 2;
  while (p < n) p <<= 1;
  return p;
}
inline size_t fold_lds_bytes(uint32_t entries) { return (size_t)entries * 16 + (2 * FOLD_QPW + 4) * sizeof(int32_t); }

// ascending float order as unsigned order, -0.0 and +0.0 on one key
__device__ __forceinline__ uint32_t dist_key(uint32_t bits) {
  if (bits == 0x80000000u) bits = 0;
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

// grid: ceil(nq / qpw) workgroups of FOLD_THREADS.  LDS: ids [E] | keys [E] | distance bits [E] | counts, E = qpw * seg.
__global__ __launch_bounds__(FOLD_THREADS) void fold_kernel(FoldArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t E = a.qpw * a.seg;
  int64_t *s_id = (int64_t *)smem;
  uint32_t *s_key = (uint32_t *)(smem + (size_t)E * 8);
  uint32_t *s_bits = s_key + E;
  int32_t *s_cr = (int32_t *)(s_bits + E);
  int32_t *s_ca = s_cr + FOLD_QPW;
  uint32_t *s_n2 = (uint32_t *)(s_ca + FOLD_QPW);
  const uint32_t t = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * a.qpw;

  if (t == 0) *s_n2 = 2;
  __syncthreads();
  if (t < a.qpw) {
    const int64_t q = q0 + t;
    int32_t cr = 0, ca = 0;
    if (q < a.nq) {
      if (a.r_cnt) cr = min(max(a.r_cnt[q], 0), a.k);
      ca = min(max(a.a_cnt[q], 0), a.k_a);
    }
    s_cr[t] = cr;
    s_ca[t] = ca;
    uint32_t n2 = 2;
    while (n2 < (uint32_t)(cr + ca)) n2 <<= 1;
    atomicMax(s_n2, n2);
  }
  __syncthreads();
  const uint32_t n2 = *s_n2;  // <= seg: cr + ca <= k + k_a
  const uint32_t used = a.qpw * n2, sh = (uint32_t)__ffs(n2) - 1;

  // the union of each query, padded to n2 with entries that sort last
  for (uint32_t e = t; e < used; e += FOLD_THREADS) {
    const uint32_t g = e >> sh, i = e & (n2 - 1);
    const int64_t q = q0 + g;
    const uint32_t cr = (uint32_t)s_cr[g], ca = (uint32_t)s_ca[g];
    uint32_t key = 0xffffffffu, bits = 0;
    int64_t id = INT64_MAX;
    if (i < cr) {
      bits = __float_as_uint(a.r_dist[(size_t)q * a.k + i]);
      id = a.r_ids[(size_t)q * a.k + i];
      key = dist_key(bits);
    } else if (i < cr + ca) {
      bits = __float_as_uint(a.a_dist[(size_t)q * a.k_a + (i - cr)]);
      id = a.a_ids[(size_t)q * a.k_a + (i - cr)];
      key = dist_key(bits);
    }
    s_key[e] = key;
    s_bits[e] = bits;
    s_id[e] = id;
  }
  __syncthreads();

  // every aligned segment of n2 entries ascending by (key, id)
  for (uint32_t size = 2; size <= n2; size <<= 1)
    for (uint32_t str = size >> 1; str > 0; str >>= 1) {
      for (uint32_t p = t; p < used / 2; p += FOLD_THREADS) {
        uint32_t lo, hi;
        if (str == size >> 1) {  // the mirrored first step of a merge
          const uint32_t blk = p / str, off = p & (str - 1);
          lo = blk * size + off;
          hi = blk * size + size - 1 - off;
        } else {
          lo = 2 * p - (p & (str - 1));
          hi = lo + str;
        }
        const uint32_t kl = s_key[lo], kh = s_key[hi];
        const int64_t il = s_id[lo], ih = s_id[hi];
        if (kh < kl || (kh == kl && ih < il)) {
          const uint32_t bl = s_bits[lo], bh = s_bits[hi];
          s_key[lo] = kh;
          s_key[hi] = kl;
          s_id[lo] = ih;
          s_id[hi] = il;
          s_bits[lo] = bh;
          s_bits[hi] = bl;
        }
      }
      __syncthreads();
    }

  // the best k of each query, one thread per output slot of the workgroup; slots past the count are zeros
  for (uint32_t e = t; e < a.qpw * (uint32_t)a.k; e += FOLD_THREADS) {
    const uint32_t g = e / (uint32_t)a.k, i = e - g * (uint32_t)a.k;
    const int64_t q = q0 + g;
    if (q >= a.nq) break;  // (g grows with e)
    const uint32_t m = min((uint32_t)(s_cr[g] + s_ca[g]), (uint32_t)a.k);
    a.o_dist[(size_t)q * a.k + i] = i < m ? __uint_as_float(s_bits[g * n2 + i]) : 0.0f;
    a.o_ids[(size_t)q * a.k + i] = i < m ? s_id[g * n2 + i] : 0;
    if (i == 0) a.o_cnt[q] = (int32_t)m;
  }
}

// rows [m][d] of a device-resident store read through a position list -> the set's query buffer, the layout a search
// uploads.  One thread per 16-byte piece when d is a multiple of 4 (hipMalloc's alignment does the rest), else per float.
__global__ void gather_rows_kernel(const float *__restrict__ rows, const int64_t *__restrict__ pos, int64_t m, int d, int vec,
                                   float *__restrict__ out) {
  const int per = vec ? d >> 2 : d;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m * per) return;
  const int64_t r = e / per;
  const int c = (int)(e - r * per);
  if (vec) ((float4 *)(out + r * d))[c] = ((const float4 *)(rows + pos[r] * d))[c];
  else out[r * d + c] = rows[pos[r] * d + c];
}

// the running answer of a chunk: two (dist, ids, cnt) buffers that swap roles at every fold
struct Running {
  Buf dist[2], ids[2], cnt[2];
  int cur = -1;  // the buffer that holds the answer; -1: nothing folded yet
  int reserve(int32_t nq, int32_t k) {
    for (int b = 0; b < 2; ++b) {
      ITRY(dist[b].reserve((size_t)nq * k * sizeof(float)));
      ITRY(ids[b].reserve((size_t)nq * k * sizeof(int64_t)));
      ITRY(cnt[b].reserve((size_t)nq * sizeof(int32_t)));
    }
    cur = -1;
    return IVF_OK;
  }
  // folds the answers a_* ([nq][k_a], [nq], device) of one member in
  int fold(int32_t nq, int32_t k, int32_t k_a, const float *a_dist, const int64_t *a_ids, const int32_t *a_cnt, hipStream_t st) {
    const int nxt = cur < 0 ? 0 : cur ^ 1;
    FoldArgs a;
    a.r_dist = cur < 0 ? nullptr : dist[cur].as<float>();
    a.r_ids = cur < 0 ? nullptr : ids[cur].as<int64_t>();
    a.r_cnt = cur < 0 ? nullptr : cnt[cur].as<int32_t>();
    a.a_dist = a_dist;
    a.a_ids = a_ids;
    a.a_cnt = a_cnt;
    a.o_dist = dist[nxt].as<float>();
    a.o_ids = ids[nxt].as<int64_t>();
    a.o_cnt = cnt[nxt].as<int32_t>();
    a.nq = nq;
    a.k = k;
    a.k_a = k_a;
    a.seg = pow2_at_least((uint32_t)(k + k_a));
    a.qpw = std::max<uint32_t>(1, std::min<uint32_t>(FOLD_QPW, FOLD_ENTRIES / a.seg));
    hipLaunchKernelGGL(fold_kernel, dim3((unsigned)((nq + a.qpw - 1) / a.qpw)), dim3(FOLD_THREADS), fold_lds_bytes(a.qpw * a.seg), st, a);
    ITRY(hipGetLastError());
    cur = nxt;
    return IVF_OK;
  }
  // the answer of the chunk -> host; with nothing folded: counts 0
  int download(int32_t nq, int32_t k, float *out_dist, int64_t *out_ids, int32_t *out_counts) {
    if (cur < 0) {
      cur = 0;
      ITRY(hipMemset(dist[0].p, 0, (size_t)nq * k * sizeof(float)));
      ITRY(hipMemset(ids[0].p, 0, (size_t)nq * k * sizeof(int64_t)));
      ITRY(hipMemset(cnt[0].p, 0, (size_t)nq * sizeof(int32_t)));
    }
    ITRY(hipMemcpy(out_dist, dist[cur].p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost));
    ITRY(hipMemcpy(out_ids, ids[cur].p, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost));
    ITRY(hipMemcpy(out_counts, cnt[cur].p, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost));
    return IVF_OK;
  }
  // the answer of the chunk -> the caller's device buffers; with nothing folded: counts 0
  int copy_out(int32_t nq, int32_t k, float *d_dist, int64_t *d_ids, int32_t *d_counts) {
    if (cur < 0) {
      ITRY(hipMemset(d_dist, 0, (size_t)nq * k * sizeof(float)));
      ITRY(hipMemset(d_ids, 0, (size_t)nq * k * sizeof(int64_t)));
      ITRY(hipMemset(d_counts, 0, (size_t)nq * sizeof(int32_t)));
      return IVF_OK;
    }
    ITRY(hipMemcpy(d_dist, dist[cur].p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToDevice));
    ITRY(hipMemcpy(d_ids, ids[cur].p, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToDevice));
    ITRY(hipMemcpy(d_counts, cnt[cur].p, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToDevice));
    return IVF_OK;
  }
};

struct Member {
  int32_t kind = 0;
  void *h = nullptr;
};

}  // namespace

struct shardset {
  int device = 0, dimension = 0, metric = 0;
  std::vector<Member> members;
  Buf dq, a_dist, a_ids, a_cnt;
  Running run;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  int64_t h2d = 0, d2h_ctl = 0, d2h_res = 0, ctl_up = 0;  // (ctl_up: the part of d2h_ctl that went up, ivf_device_rows.h)
  float t_search = 0, t_fold = 0;
  std::shared_ptr<void> by_id;  // the by-id scratch of this set (faiss_by_id.hip), freed with it
  ~shardset() {
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace {

int check_limits(int32_t nq, int32_t k, int32_t nprobe) {
  if (nq < 1) return fail(IVF_EINVAL, "nq must be positive");
  if (k < 1 || k > MAX_K) return fail(IVF_EINVAL, "k must be in 1..1024");
  if (nprobe < 1 || nprobe > MAX_NPROBE) return fail(IVF_EINVAL, "nprobe must be in 1..1024");
  return IVF_OK;
}

// device, embedding dimension, metric and rows of a member
int member_shape(const Member &m, int *device, int32_t *dimension, int32_t *metric, int64_t *rows) {
  if (m.kind == FAISS_KIND_IVF_FLAT) {
    const ivf_index_t *ix = (const ivf_index_t *)m.h;
    if (ivf_index_info(ix, rows, dimension, metric, nullptr)) return fail(IVF_EINVAL, ivf_last_error());
    *device = ivf_internal::device_of(ix);
  } else if (m.kind == FAISS_KIND_IVF_PQ) {
    const ivfpq_index_t *ix = (const ivfpq_index_t *)m.h;
    if (ivfpq_index_info(ix, rows, dimension, metric, nullptr, nullptr)) return fail(IVF_EINVAL, ivfpq_last_error());
    *device = ivfpq_internal::device_of(ix);
  } else {
    const opq_index_t *ix = (const opq_index_t *)m.h;
    if (opq_index_info(ix, rows, dimension, nullptr, metric, nullptr, nullptr)) return fail(IVF_EINVAL, opq_last_error());
    *device = opq_internal::device_of(ix);
  }
  return IVF_OK;
}

// member i searches the nq device queries into the set's shard buffer
int member_search(shardset *s, size_t i, int32_t nq, int32_t k, int32_t nprobe, int32_t ht) {
  const Member &m = s->members[i];
  float *dd = s->a_dist.as<float>();
  int64_t *di = s->a_ids.as<int64_t>();
  int32_t *dc = s->a_cnt.as<int32_t>();
  const float *q = s->dq.as<float>();
  int rc;
  const char *msg;
  int64_t ctl, up;
  if (m.kind == FAISS_KIND_IVF_FLAT) {
    rc = ivf_internal::search_device_out((ivf_index_t *)m.h, nq, q, k, nprobe, dd, di, dc);
    msg = ivf_last_error();
    ctl = ivf_internal::last_control_bytes((ivf_index_t *)m.h);
    up = ivf_internal::last_control_upload_bytes((ivf_index_t *)m.h);
  } else if (m.kind == FAISS_KIND_IVF_PQ) {
    rc = ivfpq_internal::search_device_out((ivfpq_index_t *)m.h, nq, q, k, nprobe, ht, dd, di, dc);
    msg = ivfpq_last_error();
    ctl = ivfpq_internal::last_control_bytes((ivfpq_index_t *)m.h);
    up = ivfpq_internal::last_control_upload_bytes((ivfpq_index_t *)m.h);
  } else {
    rc = opq_internal::search_device_out((opq_index_t *)m.h, nq, q, k, nprobe, ht, dd, di, dc);
    msg = opq_last_error();
    ctl = opq_internal::last_control_bytes((opq_index_t *)m.h);
    up = opq_internal::last_control_upload_bytes((opq_index_t *)m.h);
  }
  if (rc) return fail(rc, "member " + std::to_string(i) + ": " + msg);
  s->d2h_ctl += ctl;
  s->ctl_up += up;
  return IVF_OK;
}

// one chunk of <= CHUNK queries: upload (or, with pos, the gather out of the store whose first row is `queries`), every
// member's search and fold, download (or, with out_on_device, the copy into the caller's device buffers)
int search_chunk(shardset *s, int32_t nq, const float *queries, const int64_t *pos, int32_t k, int32_t nprobe, int32_t ht,
                 float *out_dist, int64_t *out_ids, int32_t *out_counts, bool out_on_device) {
  hipStream_t st = 0;
  const size_t qbytes = (size_t)nq * s->dimension * sizeof(float);
  ITRY(s->dq.reserve(qbytes));
  ITRY(s->a_dist.reserve((size_t)nq * k * sizeof(float)));
  ITRY(s->a_ids.reserve((size_t)nq * k * sizeof(int64_t)));
  ITRY(s->a_cnt.reserve((size_t)nq * sizeof(int32_t)));
  if (int rc = s->run.reserve(nq, k)) return rc;
  if (pos) {
    const int d = s->dimension, vec = d % 4 == 0 ? 1 : 0;
    const int64_t pieces = (int64_t)nq * (vec ? d >> 2 : d);
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, st, queries, pos, (int64_t)nq, d, vec,
                       s->dq.as<float>());
    ITRY(hipGetLastError());
  } else {
    ITRY(hipMemcpy(s->dq.p, queries, qbytes, hipMemcpyHostToDevice));
    s->h2d += (int64_t)qbytes;
  }
  for (size_t i = 0; i < s->members.size(); ++i) {
    ITRY(hipEventRecord(s->ev[0], st));
    if (int rc = member_search(s, i, nq, k, nprobe, ht)) return rc;
    ITRY(hipEventRecord(s->ev[1], st));
    if (int rc = s->run.fold(nq, k, k, s->a_dist.as<float>(), s->a_ids.as<int64_t>(), s->a_cnt.as<int32_t>(), st)) return rc;
    ITRY(hipEventRecord(s->ev[2], st));
    ITRY(hipEventSynchronize(s->ev[2]));  // for the two times below; the stream alone orders the next member after this fold
    float ts = 0, tf = 0;
    (void)hipEventElapsedTime(&ts, s->ev[0], s->ev[1]);
    (void)hipEventElapsedTime(&tf, s->ev[1], s->ev[2]);
    s->t_search += ts;
    s->t_fold += tf;
  }
  if (out_on_device) return s->run.copy_out(nq, k, out_dist, out_ids, out_counts);
  if (int rc = s->run.download(nq, k, out_dist, out_ids, out_counts)) return rc;
  s->d2h_res += (int64_t)nq * k * 12 + (int64_t)nq * 4;
  return IVF_OK;
}

// shardset_search over host queries, or (pos) over rows of a store into device buffers
int search_rows(shardset *set, int32_t nq, const float *queries, const int64_t *pos, int32_t k, int32_t nprobe, int32_t ht,
                float *out_dist, int64_t *out_ids, int32_t *out_counts) {
  if (!set || !queries || !out_dist || !out_ids || !out_counts) return fail(IVF_EINVAL, "null argument");
  if (int rc = check_limits(nq, k, nprobe)) return rc;
  if (int rc = shardset_internal::check_ht(set, ht)) return rc;
  ITRY(hipSetDevice(set->device));
  set->h2d = set->d2h_ctl = set->d2h_res = set->ctl_up = 0;
  set->t_search = set->t_fold = 0;
  for (int32_t q0 = 0; q0 < nq; q0 += CHUNK) {
    const int32_t m = std::min<int32_t>(CHUNK, nq - q0);
    if (int rc = search_chunk(set, m, pos ? queries : queries + (size_t)q0 * set->dimension, pos ? pos + q0 : nullptr, k, nprobe, ht,
                              out_dist + (size_t)q0 * k, out_ids + (size_t)q0 * k, out_counts + q0, pos != nullptr))
      return rc;
  }
  return IVF_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// the by-id seam (ivf_device_rows.h)
// ---------------------------------------------------------------------------------------------
int shardset_internal::check_ht(const shardset *set, int32_t ht) {
  if (ht > 0)
    for (size_t i = 0; i < set->members.size(); ++i)
      if (set->members[i].kind == FAISS_KIND_IVF_FLAT)
        return fail(IVF_EINVAL, "member " + std::to_string(i) + " is an IVF-Flat index, which has no polysemous codes: ht cannot be set");
  return IVF_OK;
}
int shardset_internal::search_store_out(shardset *set, int32_t nq, const float *d_store_rows, const int64_t *d_pos, int32_t k,
                                        int32_t nprobe, int32_t ht, float *d_dist, int64_t *d_ids, int32_t *d_counts) try {
  if (!d_pos) return fail(IVF_EINVAL, "null argument");
  return search_rows(set, nq, d_store_rows, d_pos, k, nprobe, ht, d_dist, d_ids, d_counts);
} ABI_CATCH
int shardset_internal::device_of(const shardset *set) { return set->device; }
int shardset_internal::dimension_of(const shardset *set) { return set->dimension; }
int64_t shardset_internal::last_control_bytes(const shardset *set) { return set->d2h_ctl; }
int64_t shardset_internal::last_control_upload_bytes(const shardset *set) { return set->ctl_up; }
std::shared_ptr<void> &shardset_internal::by_id_scratch(shardset *set) { return set->by_id; }

extern "C" {

const char *shardset_last_error(void) { return g_err.c_str(); }

int shardset_create(int32_t device, int32_t dimension, int32_t metric, shardset_t **out) try {
  if (!out) return fail(IVF_EINVAL, "null argument");
  if (metric < IVF_METRIC_L2 || metric > IVF_METRIC_INNER_PRODUCT) return fail(IVF_EINVAL, "unknown metric");
  if (dimension < 1) return fail(IVF_EINVAL, "dimension must be positive");
  ITRY(hipSetDevice(device));
  std::unique_ptr<shardset> s(new shardset);
  s->device = device;
  s->dimension = dimension;
  s->metric = metric;
  for (auto &e : s->ev) ITRY(hipEventCreate(&e));
  *out = s.release();
  return IVF_OK;
} ABI_CATCH

int shardset_set_members(shardset_t *set, int32_t n, const int32_t *kinds, void *const *handles) try {
  if (!set) return fail(IVF_EINVAL, "null set");
  if (n < 0) return fail(IVF_EINVAL, "n must not be negative");
  if (n > 0 && (!kinds || !handles)) return fail(IVF_EINVAL, "null argument");
  std::vector<Member> members((size_t)n);
  for (int32_t i = 0; i < n; ++i) {
    Member &m = members[(size_t)i];
    m.kind = kinds[i];
    m.h = handles[i];
    const std::string who = "member " + std::to_string(i);
    if (m.kind != FAISS_KIND_IVF_FLAT && m.kind != FAISS_KIND_IVF_PQ && m.kind != FAISS_KIND_OPQ_IVF_PQ)
      return fail(IVF_EINVAL, who + ": unknown kind " + std::to_string(m.kind));
    if (!m.h) return fail(IVF_EINVAL, who + ": null handle");
    int device = 0;
    int32_t dimension = 0, metric = 0;
    int64_t rows = 0;
    if (int rc = member_shape(m, &device, &dimension, &metric, &rows)) return rc;
    if (device != set->device)
      return fail(IVF_EINVAL, who + " is on device " + std::to_string(device) + ", the set on " + std::to_string(set->device));
    if (dimension != set->dimension)
      return fail(IVF_EINVAL, who + " has dimension " + std::to_string(dimension) + ", the set " + std::to_string(set->dimension));
    if (metric != set->metric)
      return fail(IVF_EINVAL, who + " has metric " + std::to_string(metric) + ", the set " + std::to_string(set->metric));
  }
  set->members.swap(members);
  return IVF_OK;
} ABI_CATCH

int shardset_info(const shardset_t *set, int32_t *n_members, int32_t *dimension, int32_t *metric, int64_t *rows) try {
  if (!set) return fail(IVF_EINVAL, "null set");
  if (n_members) *n_members = (int32_t)set->members.size();
  if (dimension) *dimension = set->dimension;
  if (metric) *metric = set->metric;
  if (rows) {
    int64_t total = 0;
    for (const Member &m : set->members) {
      int device = 0;
      int32_t d = 0, mt = 0;
      int64_t n = 0;
      if (int rc = member_shape(m, &device, &d, &mt, &n)) return rc;
      total += n;
    }
    *rows = total;
  }
  return IVF_OK;
} ABI_CATCH

int shardset_search(shardset_t *set, int32_t nq, const float *queries, int32_t k, int32_t nprobe, int32_t ht, float *out_dist,
                    int64_t *out_ids, int32_t *out_counts) try {
  return search_rows(set, nq, queries, nullptr, k, nprobe, ht, out_dist, out_ids, out_counts);
} ABI_CATCH

int shardset_last_stats(const shardset_t *set, int64_t *h2d_bytes, int64_t *d2h_bytes, int64_t *d2h_result_bytes, float *search_ms,
                        float *fold_ms) try {
  if (!set) return fail(IVF_EINVAL, "null set");
  if (h2d_bytes) *h2d_bytes = set->h2d;
  if (d2h_bytes) *d2h_bytes = set->d2h_res + set->d2h_ctl;
  if (d2h_result_bytes) *d2h_result_bytes = set->d2h_res;
  if (search_ms) *search_ms = set->t_search;
  if (fold_ms) *fold_ms = set->t_fold;
  return IVF_OK;
} ABI_CATCH

int shardset_compose(int32_t device, int32_t n_shards, int32_t nq, int32_t k_in, const int64_t *ids, const float *dist,
                     const int32_t *counts, int32_t k, int64_t *out_ids, float *out_dist, int32_t *out_counts) try {
  if (n_shards < 1) return fail(IVF_EINVAL, "n_shards must be positive");
  if (nq < 0) return fail(IVF_EINVAL, "nq must not be negative");
  if (k_in < 0 || k_in > MAX_K) return fail(IVF_EINVAL, "k_in must be in 0..1024");
  if (k < 1 || k > MAX_K) return fail(IVF_EINVAL, "k must be in 1..1024");
  if (nq > 0 && (!counts || !out_counts || !out_ids || !out_dist || (k_in > 0 && (!ids || !dist)))) return fail(IVF_EINVAL, "null argument");
  for (size_t e = 0; e < (size_t)n_shards * nq; ++e)
    if (counts[e] < 0 || counts[e] > k_in) return fail(IVF_EINVAL, "a shard's count is outside 0..k_in");
  if (nq == 0) return IVF_OK;
  ITRY(hipSetDevice(device));
  Buf a_dist, a_ids, a_cnt;
  Running run;
  for (int32_t q0 = 0; q0 < nq; q0 += CHUNK) {
    const int32_t m = std::min<int32_t>(CHUNK, nq - q0);
    ITRY(a_dist.reserve((size_t)m * k_in * sizeof(float)));
    ITRY(a_ids.reserve((size_t)m * k_in * sizeof(int64_t)));
    ITRY(a_cnt.reserve((size_t)m * sizeof(int32_t)));
    if (int rc = run.reserve(m, k)) return rc;
    for (int32_t s = 0; s < n_shards; ++s) {
      const size_t row = (size_t)s * nq + q0;
      if (k_in > 0) {
        ITRY(hipMemcpy(a_dist.p, dist + row * k_in, (size_t)m * k_in * sizeof(float), hipMemcpyHostToDevice));
        ITRY(hipMemcpy(a_ids.p, ids + row * k_in, (size_t)m * k_in * sizeof(int64_t), hipMemcpyHostToDevice));
      }
      ITRY(hipMemcpy(a_cnt.p, counts + row, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice));
      if (int rc = run.fold(m, k, k_in, a_dist.as<float>(), a_ids.as<int64_t>(), a_cnt.as<int32_t>(), 0)) return rc;
    }
    if (int rc = run.download(m, k, out_dist + (size_t)q0 * k, out_ids + (size_t)q0 * k, out_counts + q0)) return rc;
  }
  return IVF_OK;
} ABI_CATCH

int shardset_destroy(shardset_t *set) try {
  if (!set) return IVF_OK;
  (void)hipSetDevice(set->device);
  delete set;
  return IVF_OK;
} ABI_CATCH

}  // extern "C"
