// ivf_ann.hip -- inverted-file index with flat lists (`IVF<nlist>,Flat` in an id map) on the gfx950 matrix cores.
//
// What it replaces: the reference's Faiss queryable (ann/src/main/scala/com/twitter/ann/faiss/FaissIndexer.scala:82-92:
// index_factory -> train -> add_with_ids; QueryableIndexAdapter.scala:139-178: search with FaissRuntimeParam.nprobe),
// restricted to the coarse quantizer, its training, the inverted lists and the probed scan (include/ivf_ann.h).
//
// Shape of the computation.
//   * The coarse quantizer is the exhaustive search of dense_ann.hip over the centroids: the handle keeps them as a
//     dann_index and calls the prepared-search seam of ann_by_id_internal.h with k = nprobe (search) or k = 1 (add and
//     every k-means round).  There is no second GEMM here.
//   * The rows are kept twice: row-major fp16 in the order they were added (what an add re-lays the lists out from, and
//     what training sums), and in the lists -- one contiguous buffer in which every list starts on a 32-row block and
//     is stored in MFMA A-fragment order ([block][k-step][lane][8 halves], lane (r, h) holding x[r][16s + 8h .. +8]),
//     in (cell, id) order, beside a per-slot bias (0, -|x|^2/2 for L2, -inf for the padding of a list's last block) and
//     the slot's rank in id order.
//   * A search inverts its [nq][nprobe] probe table on the device: the (cell, query) pairs are sorted by cell and cut
//     into groups of <= 32 queries.  One workgroup per group: the group's queries are gathered once into LDS as the B
//     operand, the four waves stride over the cell's blocks, each block one coalesced 1-KiB load per k-step and one
//     v_mfma_f32_32x32x16_f16, fp32 accumulation started from the bias.  C has the query on the lane and 16 rows in
//     the accumulator registers, so the threshold test is register-local.  A cell's rows are read once per group of
//     queries that probe it, not once per query.
//   * Candidates go to a per-query survivor buffer (CAP = 8192) by one integer atomic per (lane, block) that reserves
//     as many slots as the lane has candidates.  Round 0 runs with threshold -inf: a query whose probed lists hold
//     <= CAP rows has all of them and is finished.  A query that overflowed takes the k-th largest of the CAP scores
//     it did buffer as its threshold -- a lower bound of its k-th best score, k distinct rows reach it -- and only its
//     groups are scanned again (fallback round, counted in ivf_last_stats); every row at or above the threshold is
//     emitted then, so the k best are among the survivors whatever order the workgroups appended in.
//   * Select sorts a query's survivors by (score desc, rank in id order asc): the order of dense_ann.hip's select.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/dense_ann.h"
#include "../../include/ivf_ann.h"
#include "sann_device.h"  // mix64
#include "ivf_device_rows.h"
#include "faiss_restore.h"
#include "ivf_core.h"
#include "ivf_flat_lists.h"

namespace {

// Restoring a saved index: the sum of squares of stored fp16 rows, by the second half of store_rows_kernel exactly -- one
// wave per row, lane l sums components l, l + 64, ... in fp64, then the same shuffle tree -- so that a restored row carries
// the bits it carried when it was added.
__global__ void stored_sumsq_kernel(const _Float16 *__restrict__ flat, int64_t n, int d, float *__restrict__ sumsq) {
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  double ss16 = 0;
  for (int k = lane; k < d; k += 64) {
    const float back = (float)flat[row * d + k];
    ss16 += (double)back * (double)back;
  }
  ss16 = wave_sum(ss16);
  if (lane == 0) sumsq[row] = (float)ss16;
}
// One workgroup per cell: component k of the mean is summed by one thread over the cell's rows in position order, in
// fp64 -- a fixed order, no floating-point atomics.  InnerProduct / Cosine: the mean is scaled to unit length, its
// squared norm summed by one thread in component order.  A cell without rows keeps its centroid.
__global__ __launch_bounds__(256) void mean_kernel(const _Float16 *__restrict__ flat, int d, int metric,
                                                   const uint32_t *__restrict__ ord, const uint32_t *__restrict__ start,
                                                   const uint32_t *__restrict__ sizes, float *__restrict__ cent) {
  __shared__ double sq[MAX_D];
  __shared__ double s_scale;
  const uint32_t c = blockIdx.x, n = sizes[c], j0 = start[c];
  if (n == 0) return;
  double mean[MAX_D / 256];
#pragma unroll
  for (int u = 0; u < MAX_D / 256; ++u) {
    const int k = threadIdx.x + u * 256;
    double acc = 0;
    if (k < d)
      for (uint32_t j = 0; j < n; ++j) acc += (double)(float)flat[(size_t)ord[j0 + j] * d + k];
    mean[u] = acc / (double)n;
    if (k < d) sq[k] = mean[u] * mean[u];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double scale = 1.0;
    if (metric != IVF_METRIC_L2) {
      double ss = 0;
      for (int k = 0; k < d; ++k) ss += sq[k];
      if (ss > 0) scale = 1.0 / sqrt(ss);
    }
    s_scale = scale;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < MAX_D / 256; ++u) {
    const int k = threadIdx.x + u * 256;
    if (k < d) cent[(size_t)c * d + k] = (float)(mean[u] * s_scale);
  }
}

// ---------------------------------------------------------------------------------------------
// the probed scan
// ---------------------------------------------------------------------------------------------
struct ScanArgs {
  const _Float16 *lf;     // list fragments
  const float *lbias;     // per slot
  const uint32_t *boff;   // first block of a cell's list
  const uint32_t *nblk;   // its blocks
  const _Float16 *qf;     // query fragments of the chunk, S = d / 16
  const Group *groups;
  const uint32_t *pair_q; // queries of the pairs sorted by cell
  const float *tau;       // [nq]: emit scores >= tau; +inf = the query is finished
  uint32_t *cnt;          // [nq]
  Survivor *surv;         // [nq][CAP]
  int S;
};

__global__ __launch_bounds__(256) void scan_kernel(ScanArgs a) {
  extern __shared__ half8 sq[];  // [S][64]: the group's queries as the B operand
  __shared__ int s_q[32];
  __shared__ float s_tau[32];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, S = a.S;
  const Group g = a.groups[blockIdx.x];
  if (t < 32) {
    const int q = t < (int)g.count ? (int)a.pair_q[g.p0 + t] : -1;
    s_q[t] = q;
    s_tau[t] = q >= 0 ? a.tau[q] : INFINITY;
  }
  __syncthreads();
  const int myq = s_q[lane & 31];
  const float thr = s_tau[lane & 31];
  if (!__syncthreads_or(thr < INFINITY)) return;  // a fallback round: every query of this group is finished
  for (int i = t; i < S * 64; i += 256) {
    const int s = i >> 6, l = i & 63, q = s_q[l & 31];
    half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (q >= 0) v = *(const half8 *)&a.qf[((((size_t)(q >> 5) * S + s) * 64) + (l >> 5) * 32 + (q & 31)) * 8];
    sq[i] = v;
  }
  __syncthreads();
  const uint32_t b0 = a.boff[g.cell], nb = a.nblk[g.cell];
  for (uint32_t blk = w; blk < nb; blk += 4) {
    const size_t gb = (size_t)b0 + blk;
    // row of accumulator register i on this lane: (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
    const float *bp = a.lbias + gb * 32 + 4 * (lane >> 5);
    float16v acc;
#pragma unroll
    for (int i4 = 0; i4 < 4; ++i4) {
      const float4 bv = *(const float4 *)(bp + 8 * i4);
      acc[4 * i4 + 0] = bv.x;
      acc[4 * i4 + 1] = bv.y;
      acc[4 * i4 + 2] = bv.z;
      acc[4 * i4 + 3] = bv.w;
    }
    const half8 *ap = (const half8 *)a.lf + gb * S * 64 + lane;
    for (int s = 0; s < S; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ap[(size_t)s * 64], sq[s * 64 + lane], acc, 0, 0, 0);
    if (myq < 0) continue;
    // padding rows carry the bias -inf: they pass no threshold, not even -inf
    uint32_t pass = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) pass |= (uint32_t)(acc[i] >= thr && acc[i] > -INFINITY) << i;
    if (pass == 0) continue;
    uint32_t pos = atomicAdd(&a.cnt[myq], (uint32_t)__popc(pass));
    const uint32_t slot0 = (uint32_t)(gb * 32) + 4u * (uint32_t)(lane >> 5);
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (pass >> i & 1) {
        if (pos < (uint32_t)CAP) a.surv[(size_t)myq * CAP + pos] = Survivor{acc[i], slot0 + (i & 3) + 8 * (i >> 2)};
        ++pos;
      }
  }
}

}  // namespace

struct ivf_index : IvfBase {
  // the rows in the order added
  Buf flat, sumsq;
  // the lists' payload
  Buf lf, lbias;
  // per-call scratch: the queries, and the groups of a search
  Buf qf;
  GroupTable gt;
};

namespace {

int new_index(int32_t device, int32_t metric, int32_t d, int32_t nlist, std::unique_ptr<ivf_index> &ix) {
  ITRY(hipSetDevice(device));
  ix.reset(new ivf_index);
  if (int rc = init_base(ix.get(), device, metric, d, nlist)) return rc;
  ITRY(hipFuncSetAttribute((const void *)select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SELECT_LDS));
  return IVF_OK;
}

// all lists again from the rows in the order added: blocks of 32 rows as A fragments, beside the bias and the rank
int layout_lists(ivf_index *ix) {
  return layout_lists(ix, 32, [ix](size_t slots) -> int {
    const int d = ix->d;
    ITRY(ix->lf.reserve(slots * d * sizeof(_Float16)));
    ITRY(ix->lbias.reserve(slots * sizeof(float)));
    ITRY(hipMemset(ix->lf.p, 0, slots * d * sizeof(_Float16)));
    hipLaunchKernelGGL(fill_kernel, dim3(blocks_for((int64_t)slots)), dim3(256), 0, 0, ix->lbias.as<float>(), (int64_t)slots, -INFINITY);
    ITRY(hipGetLastError());
    hipLaunchKernelGGL(scatter_rows_kernel, dim3(blocks_for(ix->n, 4)), dim3(256), 0, 0, ix->flat.as<_Float16>(), ix->sumsq.as<float>(),
                       ix->n, d, ix->metric, ix->cell_sorted.as<uint32_t>(), ix->ord.as<uint32_t>(), ix->perm.as<uint32_t>(),
                       ix->start.as<uint32_t>(), ix->boff.as<uint32_t>(), ix->lf.as<_Float16>(), ix->lbias.as<float>(),
                       ix->lrank.as<uint32_t>());
    ITRY(hipGetLastError());
    return IVF_OK;
  });
}

int build_coarse(ivf_index *ix, const float *d_cent, bool stored = false) {
  dann_index *c = nullptr;
  DCALL(ann_by_id::dann_build_device(ix->device, ix->metric, ix->nlist, ix->d, d_cent, &c, stored));
  if (ix->coarse) (void)dann_index_destroy(ix->coarse);
  ix->coarse = c;
  return IVF_OK;
}

// One chunk of a search.  out_on_device: out_dist / out_ids / out_counts are device buffers, which the select launch writes
// itself; otherwise it writes the index's own and finish_chunk brings them to the host.
int search_chunk(ivf_index *ix, int32_t q0, int32_t nq, const float *queries, bool on_device, const int64_t *pos, int32_t k,
                 int32_t nprobe, float *out_dist, int64_t *out_ids, int32_t *out_counts, bool out_on_device) {
  const int d = ix->d, S = d >> 4;
  hipStream_t st = 0;
  const int nq_pad = (nq + 31) / 32 * 32;
  ITRY(ix->qf.reserve((size_t)nq_pad * d * sizeof(_Float16) * 2));  // the fp16 rows, then the scan's fragments
  _Float16 *q16 = ix->qf.as<_Float16>(), *qfrag = q16 + (size_t)nq_pad * d;
  if (int rc = probe_chunk(ix, q0, nq, queries, on_device, pos, k, nprobe, q16, qfrag)) return rc;
  if (int rc = build_groups(ix, ix->gt)) return rc;
  const uint32_t n_groups = ix->gt.n_groups;

  // scan rounds
  ScanArgs a;
  a.lf = ix->lf.as<_Float16>();
  a.lbias = ix->lbias.as<float>();
  a.boff = ix->boff.as<uint32_t>();
  a.nblk = ix->nblk.as<uint32_t>();
  a.qf = qfrag;
  a.groups = ix->gt.groups.as<Group>();
  a.pair_q = ix->pair_q_s.as<uint32_t>();
  a.tau = ix->tau.as<float>();
  a.cnt = ix->cnt.as<uint32_t>();
  a.surv = ix->surv.as<Survivor>();
  a.S = S;
  int rounds = 0;
  if (int rc = scan_rounds(ix, nq, k, [&](int, hipStream_t s) -> int {
        if (ix->n > 0) {
          hipLaunchKernelGGL(scan_kernel, dim3(n_groups), dim3(256), (size_t)S * 64 * sizeof(half8), s, a);
          ITRY(hipGetLastError());
        }
        return IVF_OK;
      }, &rounds))
    return rc;

  hipLaunchKernelGGL(select_kernel, dim3(nq), dim3(512), SELECT_LDS, st, ix->surv.as<Survivor>(), ix->done_cnt.as<uint32_t>(),
                     ix->qsumsq.as<float>(), ix->lrank.as<uint32_t>(), ix->ids_sorted.as<int64_t>(), ix->metric, k,
                     out_on_device ? out_dist : ix->o_dist.as<float>(), out_on_device ? out_ids : ix->o_ids.as<int64_t>(),
                     out_on_device ? out_counts : ix->o_cnt.as<int32_t>());
  ITRY(hipGetLastError());
  if (out_on_device) return finish_chunk(ix, nq, k, rounds, nullptr, nullptr, nullptr);
  return finish_chunk(ix, nq, k, rounds, out_dist, out_ids, out_counts);
}

// ivf_search, over host queries into host buffers or over device queries into device buffers; pos != NULL: the device
// queries are the rows pos[0 .. nq) of the store whose first row is `queries` (probe_chunk), a chunk's positions at pos + q0
int search_rows(ivf_index *ix, int32_t nq, const float *queries, int32_t k, int32_t nprobe, float *out_dist, int64_t *out_ids,
                int32_t *out_counts, bool on_device, const int64_t *pos = nullptr) {
  if (!ix || !queries || !out_dist || !out_ids || !out_counts) return fail(IVF_EINVAL, "null argument");
  if (int rc = search_begin(ix, nq, k, &nprobe)) return rc;
  return search_chunks(ix, nq, [&](int32_t q0, int32_t m) -> int {
    return search_chunk(ix, q0, m, pos ? queries : queries + (size_t)q0 * ix->d, on_device, pos ? pos + q0 : nullptr, k, nprobe,
                        out_dist + (size_t)q0 * k, out_ids + (size_t)q0 * k, out_counts + q0, on_device);
  });
}

// ivf_index_train, over host rows or over rows that are on the device
int train_rows(int32_t device, int32_t metric, int32_t d, int32_t nlist, int64_t n_train, const float *train_vectors,
               bool on_device, int32_t niter, uint64_t seed, ivf_index_t **out) {
  if (!train_vectors || !out) return fail(IVF_EINVAL, "null argument");
  if (int rc = check_shape(metric, d, nlist)) return rc;
  if (n_train < nlist) return fail(IVF_EINVAL, "n_train must be at least nlist");
  if (n_train >= ((int64_t)1 << 31)) return fail(IVF_EINVAL, "n_train out of range");
  if (niter < -1) return fail(IVF_EINVAL, "niter must be -1 (initial picks), 0 (20 rounds) or a number of rounds");
  const int rounds = niter == 0 ? 20 : niter == -1 ? 0 : niter;
  std::unique_ptr<ivf_index> ix;
  if (int rc = new_index(device, metric, d, nlist, ix)) return rc;
  // the training rows, prepared as stored rows are; they go with this call
  Buf tflat, tsumsq, picks_d, cent;
  ITRY(tflat.reserve((size_t)n_train * d * sizeof(_Float16)));
  ITRY(tsumsq.reserve((size_t)n_train * sizeof(float)));
  if (int rc = upload_rows(ix.get(), train_vectors, on_device, n_train, tflat.as<_Float16>(), tsumsq.as<float>())) return rc;
  // initial centroids: rows mix64(seed + t) mod n_train, t = 0, 1, ..., without repetition
  std::vector<int64_t> picks;
  picks.reserve((size_t)nlist);
  std::unordered_set<int64_t> seen;
  for (uint64_t t = 0; (int)picks.size() < nlist; ++t) {
    const int64_t r = (int64_t)(sann::mix64(seed + t) % (uint64_t)n_train);
    if (seen.insert(r).second) picks.push_back(r);
  }
  ITRY(picks_d.reserve((size_t)nlist * 8));
  ITRY(hipMemcpy(picks_d.p, picks.data(), (size_t)nlist * 8, hipMemcpyHostToDevice));
  ITRY(cent.reserve((size_t)nlist * d * sizeof(float)));
  hipLaunchKernelGGL(pick_rows_kernel, dim3(blocks_for((int64_t)nlist * d)), dim3(256), 0, 0, tflat.as<_Float16>(),
                     picks_d.as<int64_t>(), nlist, d, cent.as<float>());
  ITRY(hipGetLastError());
  if (metric == IVF_METRIC_INNER_PRODUCT) {
    hipLaunchKernelGGL(unit_rows_kernel, dim3(blocks_for(nlist, 4)), dim3(256), 0, 0, cent.as<float>(), nlist, d);
    ITRY(hipGetLastError());
  }
  ITRY(hipDeviceSynchronize());
  if (int rc = build_coarse(ix.get(), cent.as<float>())) return rc;
  ITRY(ix->cell.reserve((size_t)n_train * 4));
  for (int it = 0; it < rounds; ++it) {
    if (int rc = assign_rows(ix.get(), tflat.as<_Float16>(), tsumsq.as<float>(), n_train, ix->cell.as<int32_t>())) return rc;
    if (int rc = segment_by_cell(ix.get(), nullptr, n_train)) return rc;
    hipLaunchKernelGGL(mean_kernel, dim3(nlist), dim3(256), 0, 0, tflat.as<_Float16>(), d, metric, ix->ord.as<uint32_t>(),
                       ix->start.as<uint32_t>(), ix->sizes.as<uint32_t>(), cent.as<float>());
    ITRY(hipGetLastError());
    ITRY(hipDeviceSynchronize());
    if (int rc = build_coarse(ix.get(), cent.as<float>())) return rc;
  }
  // the index starts empty
  ITRY(hipMemset(ix->sizes.p, 0, (size_t)nlist * 4));
  ITRY(hipMemset(ix->start.p, 0, (size_t)nlist * 4));
  *out = ix.release();
  return IVF_OK;
}

}  // namespace

int ivf_internal::train_device(int32_t device, int32_t metric, int32_t d, int32_t nlist, int64_t n_train, const float *d_rows,
                               int32_t niter, uint64_t seed, ivf_index **out) try {
  return train_rows(device, metric, d, nlist, n_train, d_rows, true, niter, seed, out);
} ABI_CATCH

int ivf_internal::search_device_out(ivf_index *ix, int32_t nq, const float *d_queries, int32_t k, int32_t nprobe, float *d_dist,
                                    int64_t *d_ids, int32_t *d_counts) try {
  return search_rows(ix, nq, d_queries, k, nprobe, d_dist, d_ids, d_counts, true);
} ABI_CATCH

ivf_hq::State *ivf_internal::hnsw_quantizer(ivf_index *ix) { return hq_state(ix); }  // ivf_hnsw_quantizer_internal.h

int ivf_internal::search_store_out(ivf_index *ix, int32_t nq, const float *d_store_rows, const int64_t *d_pos, int32_t k,
                                   int32_t nprobe, float *d_dist, int64_t *d_ids, int32_t *d_counts) try {
  if (!d_pos) return fail(IVF_EINVAL, "null argument");
  return search_rows(ix, nq, d_store_rows, k, nprobe, d_dist, d_ids, d_counts, true, d_pos);
} ABI_CATCH

int ivf_internal::device_of(const ivf_index *ix) { return ix->device; }
int64_t ivf_internal::last_control_bytes(const ivf_index *ix) { return ix->last_ctl; }
int64_t ivf_internal::last_control_upload_bytes(const ivf_index *ix) { return ix->last_ctl_up; }
std::shared_ptr<void> &ivf_internal::by_id_scratch(ivf_index *ix) { return ix->by_id; }

// ---------------------------------------------------------------------------------------------
// restoring a saved index (faiss_restore.h)
// ---------------------------------------------------------------------------------------------
int64_t ivf_internal::restore_slab_rows(int32_t d) { return std::max<int64_t>(1, (int64_t)(32 << 20) / (d * 2 + 12)); }

int ivf_internal::restore_begin(int32_t device, int32_t metric, int32_t d, int32_t nlist, const float *centroids, int32_t ids_mode,
                                int64_t n, ivf_index **out) try {
  if (!centroids || !out) return fail(IVF_EINVAL, "null argument");
  if (int rc = check_shape(metric, d, nlist)) return rc;
  if (int rc = check_restore(ids_mode, n)) return rc;
  std::unique_ptr<ivf_index> ix;
  if (int rc = new_index(device, metric, d, nlist, ix)) return rc;
  Buf cent;
  ITRY(cent.reserve((size_t)nlist * d * sizeof(float)));
  ITRY(hipMemcpy(cent.p, centroids, (size_t)nlist * d * sizeof(float), hipMemcpyHostToDevice));
  if (int rc = build_coarse(ix.get(), cent.as<float>(), true)) return rc;
  ITRY(ix->flat.reserve((size_t)n * d * sizeof(_Float16)));
  ITRY(ix->sumsq.reserve((size_t)n * 4));
  if (int rc = restore_open(ix.get(), ids_mode, n)) return rc;
  *out = ix.release();
  return IVF_OK;
} ABI_CATCH

int ivf_internal::restore_stage(ivf_index *ix, int64_t m, int64_t **ids, int32_t **cells, uint16_t **rows16) try {
  return restore_staging(ix, m, ix ? restore_slab_rows(ix->d) : 0, ix ? (size_t)ix->d * sizeof(_Float16) : 0, ids, cells, (void **)rows16);
} ABI_CATCH

int ivf_internal::restore_slab(ivf_index *ix, int64_t r0, int64_t m) try {
  if (int rc = restore_rows(ix, r0, m, ix ? ix->flat.p : nullptr)) return rc;
  hipLaunchKernelGGL(stored_sumsq_kernel, dim3(blocks_for(m, 4)), dim3(256), 0, 0, ix->flat.as<_Float16>() + (size_t)r0 * ix->d, m,
                     ix->d, ix->sumsq.as<float>() + r0);
  ITRY(hipGetLastError());
  ITRY(hipDeviceSynchronize());
  ix->rs.done = r0 + m;
  return IVF_OK;
} ABI_CATCH

int ivf_internal::restore_end(ivf_index *ix) try {
  if (int rc = restore_close(ix)) return rc;
  return ix->n > 0 ? layout_lists(ix) : IVF_OK;
} ABI_CATCH

int ivf_internal::export_rows(const ivf_index *ix, int64_t r0, int64_t m, int64_t *ids, int32_t *cells, uint16_t *rows16) try {
  return export_columns(ix, r0, m, ids, cells, rows16, ix ? ix->flat.p : nullptr, ix ? (size_t)ix->d * sizeof(_Float16) : 0);
} ABI_CATCH

int ivf_internal::ids_mode(const ivf_index *ix) { return ix->ids_mode; }

extern "C" {

const char *ivf_last_error(void) { return g_err.c_str(); }

int ivf_index_load(int32_t device, int32_t metric, int32_t d, int32_t nlist, const float *centroids, ivf_index_t **out) try {
  if (!centroids || !out) return fail(IVF_EINVAL, "null argument");
  if (int rc = check_shape(metric, d, nlist)) return rc;
  std::unique_ptr<ivf_index> ix;
  if (int rc = new_index(device, metric, d, nlist, ix)) return rc;
  Buf cent;
  ITRY(cent.reserve((size_t)nlist * d * sizeof(float)));
  ITRY(hipMemcpy(cent.p, centroids, (size_t)nlist * d * sizeof(float), hipMemcpyHostToDevice));
  if (int rc = build_coarse(ix.get(), cent.as<float>())) return rc;
  *out = ix.release();
  return IVF_OK;
} ABI_CATCH

int ivf_index_train(int32_t device, int32_t metric, int32_t d, int32_t nlist, int64_t n_train, const float *train_vectors,
                    int32_t niter, uint64_t seed, ivf_index_t **out) try {
  return train_rows(device, metric, d, nlist, n_train, train_vectors, false, niter, seed, out);
} ABI_CATCH

int ivf_index_add(ivf_index_t *ix, int64_t n, const float *vectors, const int64_t *ids) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (n < 0) return fail(IVF_EINVAL, "n must not be negative");
  if (int rc = check_ids_rule(ix, ids != nullptr)) return rc;
  if (n == 0) return IVF_OK;
  if (!vectors) return fail(IVF_EINVAL, "null vectors");
  if (int rc = grow_rows(ix, n)) return rc;
  const int64_t n_old = ix->n, total = n_old + n;
  const int d = ix->d;
  ITRY(ix->flat.grow_keep((size_t)n_old * d * sizeof(_Float16), (size_t)total * d * sizeof(_Float16)));
  ITRY(ix->sumsq.grow_keep((size_t)n_old * 4, (size_t)total * 4));
  _Float16 *flat = ix->flat.as<_Float16>() + (size_t)n_old * d;
  float *sumsq = ix->sumsq.as<float>() + n_old;
  if (int rc = upload_rows(ix, vectors, false, n, flat, sumsq)) return rc;
  if (int rc = assign_rows(ix, flat, sumsq, n, ix->cell.as<int32_t>() + n_old)) return rc;
  if (int rc = commit_add(ix, n, ids)) return rc;
  return layout_lists(ix);
} ABI_CATCH

int ivf_search(ivf_index_t *ix, int32_t nq, const float *queries, int32_t k, int32_t nprobe, float *out_dist, int64_t *out_ids,
               int32_t *out_counts) try {
  return search_rows(ix, nq, queries, k, nprobe, out_dist, out_ids, out_counts, false);
} ABI_CATCH

int ivf_index_info(const ivf_index_t *ix, int64_t *n, int32_t *d, int32_t *metric, int32_t *nlist) try {
  return index_info(ix, n, d, metric, nlist);
} ABI_CATCH

int ivf_index_get_centroids(const ivf_index_t *ix, float *out) try { return get_centroids(ix, out); } ABI_CATCH

int ivf_index_list_sizes(const ivf_index_t *ix, int64_t *out) try { return list_sizes(ix, out); } ABI_CATCH

int ivf_index_get_assignment(const ivf_index_t *ix, int64_t *out_ids, int32_t *out_cells) try {
  return get_assignment(ix, out_ids, out_cells);
} ABI_CATCH

int ivf_last_probes(const ivf_index_t *ix, int32_t *nq, int32_t *nprobe, int32_t *out_cells) try {
  return last_probes(ix, nq, nprobe, out_cells);
} ABI_CATCH

int ivf_last_stats(const ivf_index_t *ix, int64_t *rows_scanned, int32_t *rounds, float *coarse_ms, float *scan_ms,
                   float *select_ms) try {
  return last_stats(ix, rows_scanned, rounds, coarse_ms, scan_ms, select_ms);
} ABI_CATCH

int ivf_index_destroy(ivf_index_t *ix) try {
  delete ix;
  return IVF_OK;
} ABI_CATCH

}  // extern "C"
