// grouped_ann.hip -- the grouped index (include/grouped_ann.h): the IVF-Flat list machinery with the cell given by the
// caller, on the gfx950 matrix cores.
//
// What it replaces: the grouped mode of the reference's query servers (RefreshableQueryable.scala:47-55,131-177: one
// Queryable per key in a Map[Option[String], Queryable]; QueryIndexThriftController.scala:42-57: query.key picks the map
// entry) -- there one index, one search and one scratch set per key; here one index and one pass for a mixed-key batch.
//
// Shape of the computation.
//   * Build: the rows are prepared by store_rows_kernel and laid out by ivf_core.h's layout_lists with cell = group: one
//     contiguous buffer in which every group starts on a 32-row block, rows as MFMA A fragments in (group, id) order, beside
//     the per-slot bias and the slot's rank in id order (ivf_ann.hip's header has the layout).  The row-major copy goes
//     with the build call: the index is immutable.
//   * Search, per chunk of queries: the (group, query) pairs are sorted by group (a query whose group is outside the index
//     sorts behind all others and gets no work); each group's queries are cut into tiles of <= 32, each group's list into
//     segments of SEG_BLOCKS 32-row blocks; one workgroup per (tile, segment) work item.  A group of a million rows is
//     spread over as many workgroups as it has segments, a group of forty rows costs exactly one.  Items of one segment are
//     neighbours in the grid, so the tiles that read the same rows run together.
//   * Inside a work item the arithmetic is ivf_ann.hip's scan_kernel: the tile's queries once into LDS as the B operand,
//     the four waves stride over the segment's blocks, per k-step one coalesced 1-KiB load and one
//     v_mfma_f32_32x32x16_f16, the accumulator started from the bias, the threshold test register-local, survivors to the
//     per-query buffer (CAP) by one integer atomic per (lane, block).
//   * Exactness is the argument at the top of ivf_ann.hip: any threshold that is a lower bound of the k-th best score, and
//     that k distinct rows reach, keeps the top k among the survivors whatever order the workgroups append in -- which is
//     what allows splitting a list.  A query whose group holds more than CAP rows would push every row through an atomic in
//     round 0, so round 0 opens with a sample pass for those queries alone: the first segment of the group (SEG_ROWS rows,
//     MAX_K <= SEG_ROWS <= CAP: it holds k rows and cannot overflow) is scanned with threshold -inf and the k-th largest of
//     its scores becomes the query's threshold for the pass over the whole list.  It is the k-th best of a subset, so a
//     lower bound, reached by k rows of that subset.  A query that still overflows is refined as in ivf_ann.hip (16 rounds,
//     then ELIMIT); work items whose queries are all finished exit before touching the list.
//   * Select is ivf_flat_lists.h's select_kernel: (score desc, rank in id order asc).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/grouped_ann.h"
#include "ivf_core.h"
#include "ivf_flat_lists.h"

static_assert(GANN_OK == IVF_OK && GANN_EINVAL == IVF_EINVAL && GANN_EDEVICE == IVF_EDEVICE && GANN_ELIMIT == IVF_ELIMIT &&
                  GANN_ENOMEM == IVF_ENOMEM && GANN_EINTERNAL == IVF_EINTERNAL,
              "status codes carry the numbers of ivf_ann.h");
static_assert(GANN_METRIC_L2 == IVF_METRIC_L2 && GANN_METRIC_COSINE == IVF_METRIC_COSINE &&
                  GANN_METRIC_INNER_PRODUCT == IVF_METRIC_INNER_PRODUCT,
              "metrics are those of ann_common.thrift");

namespace {

constexpr int MAX_GROUPS = 1 << 20;
constexpr int GROUP_BITS = 21;  // a sort key is a group number or n_groups itself ("no such group"): [0, 2^20]
// A segment is SEG_BLOCKS 32-row blocks, 16 per wave (DESIGN.md has the reasoning).  The sample pass needs
// MAX_K <= SEG_ROWS <= CAP.
constexpr int SEG_BLOCKS = 64;
constexpr int SEG_ROWS = SEG_BLOCKS * 32;
static_assert(SEG_ROWS >= MAX_K && SEG_ROWS <= CAP, "the first segment holds k rows and fits the survivor buffer");

struct Work {
  uint32_t p0, count;  // the queries of the tile: pairs [p0, p0 + count) of the (group, query) pairs sorted by group
  uint32_t blk0, nb;   // the segment: blocks [blk0, blk0 + nb) of the list buffer
  uint32_t sample;     // 1: the first segment of a group of more than CAP rows (the sample pass scans it); else 0
};

// ---------------------------------------------------------------------------------------------
// the work list
// ---------------------------------------------------------------------------------------------
// per group, once at build: its segments
__global__ void segments_kernel(const uint32_t *__restrict__ nblk, int n_groups, uint32_t *__restrict__ nseg) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n_groups) nseg[c] = (nblk[c] + SEG_BLOCKS - 1) / SEG_BLOCKS;
}
// one thread per query: its (group, query) pair -- a group outside the index becomes the key n_groups, behind every
// group --, the queries per group, whether its group needs the sample pass, and its share of the rows scanned
__global__ void pairs_kernel(const int32_t *__restrict__ qgroup, int nq, int n_groups, const uint32_t *__restrict__ sizes,
                             uint32_t *__restrict__ pair_cell, uint32_t *__restrict__ pair_q, uint32_t *__restrict__ per_cell,
                             uint32_t *__restrict__ qbig, unsigned long long *__restrict__ rows_scanned) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const int32_t g = qgroup[q];
  const bool known = g >= 0 && g < n_groups;
  pair_cell[q] = known ? (uint32_t)g : (uint32_t)n_groups;
  pair_q[q] = (uint32_t)q;
  uint32_t big = 0;
  if (known) {
    const uint32_t sz = sizes[g];
    atomicAdd(&per_cell[g], 1u);
    if (sz) atomicAdd(rows_scanned, (unsigned long long)sz);
    big = sz > (uint32_t)CAP;
  }
  qbig[q] = big;
}
// per group: its tiles of <= 32 queries and its (tile, segment) work items
__global__ void tiles_kernel(const uint32_t *__restrict__ per_cell, const uint32_t *__restrict__ nseg, int n_groups,
                             uint32_t *__restrict__ ntile, uint32_t *__restrict__ nwork) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_groups) return;
  const uint32_t t = (per_cell[c] + 31u) / 32u;
  ntile[c] = t;
  nwork[c] = t * nseg[c];
}
// the two totals the host needs for the grid, in one place
__global__ void totals_kernel(const uint32_t *__restrict__ tstart, const uint32_t *__restrict__ ntile,
                              const uint32_t *__restrict__ wstart, const uint32_t *__restrict__ nwork, int n_groups,
                              uint32_t *__restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    out[0] = tstart[n_groups - 1] + ntile[n_groups - 1];
    out[1] = wstart[n_groups - 1] + nwork[n_groups - 1];
  }
}
// one thread per work item: its group by binary search over the exclusive sums, then segment-major within the group
__global__ void work_kernel(uint32_t n_work, const uint32_t *__restrict__ wstart, const uint32_t *__restrict__ ntile,
                            const uint32_t *__restrict__ per_cell, const uint32_t *__restrict__ pstart,
                            const uint32_t *__restrict__ boff, const uint32_t *__restrict__ nblk,
                            const uint32_t *__restrict__ sizes, int n_groups, Work *__restrict__ work) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_work) return;
  // the last group whose first item is <= w: groups without work share their successor's start and are passed over
  int lo = 0, hi = n_groups;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (wstart[mid] <= w) lo = mid;
    else hi = mid;
  }
  const int c = lo;
  const uint32_t local = w - wstart[c], nt = ntile[c];
  const uint32_t seg = local / nt, tile = local % nt;
  Work o;
  o.p0 = pstart[c] + tile * 32u;
  o.count = min(32u, per_cell[c] - tile * 32u);
  o.blk0 = boff[c] + seg * SEG_BLOCKS;
  o.nb = min((uint32_t)SEG_BLOCKS, nblk[c] - seg * SEG_BLOCKS);
  o.sample = (sizes[c] > (uint32_t)CAP && seg == 0) ? 1u : 0u;
  work[w] = o;
}

// ---------------------------------------------------------------------------------------------
// the scan: one workgroup per (tile, segment)
// ---------------------------------------------------------------------------------------------
struct ScanArgs {
  const _Float16 *lf;      // list fragments
  const float *lbias;      // per slot
  const _Float16 *qf;      // query fragments of the chunk, S = d / 16
  const Work *work;
  const uint32_t *pair_q;  // queries of the pairs sorted by group
  const float *tau;        // [nq]: emit scores >= tau; +inf = the query is finished
  uint32_t *cnt;           // [nq]
  Survivor *surv;          // [nq][CAP]
  int S;
  int sample_pass;         // 1: only the items marked `sample` run
};

__global__ __launch_bounds__(256) void segment_scan_kernel(ScanArgs a) {
  extern __shared__ half8 sq[];  // [S][64]: the tile's queries as the B operand
  __shared__ int s_q[32];
  __shared__ float s_tau[32];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, S = a.S;
  const Work g = a.work[blockIdx.x];
  if (a.sample_pass && !g.sample) return;
  if (t < 32) {
    const int q = t < (int)g.count ? (int)a.pair_q[g.p0 + t] : -1;
    s_q[t] = q;
    s_tau[t] = q >= 0 ? a.tau[q] : INFINITY;
  }
  __syncthreads();
  const int myq = s_q[lane & 31];
  const float thr = s_tau[lane & 31];
  if (!__syncthreads_or(thr < INFINITY)) return;  // a fallback round: every query of this tile is finished
  for (int i = t; i < S * 64; i += 256) {
    const int s = i >> 6, l = i & 63, q = s_q[l & 31];
    half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (q >= 0) v = *(const half8 *)&a.qf[((((size_t)(q >> 5) * S + s) * 64) + (l >> 5) * 32 + (q & 31)) * 8];
    sq[i] = v;
  }
  __syncthreads();
  for (uint32_t blk = w; blk < g.nb; blk += 4) {
    const size_t gb = (size_t)g.blk0 + blk;
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

// after the sample pass, one workgroup per query of a group of more than CAP rows: the k-th largest of the first segment's
// scores (all buffered: SEG_ROWS <= CAP) is the threshold of the pass over the whole list; the buffer starts again
__global__ __launch_bounds__(256) void sample_threshold_kernel(const uint32_t *__restrict__ qbig, float *__restrict__ tau,
                                                               uint32_t *__restrict__ cnt, const Survivor *__restrict__ surv, int k) {
  __shared__ uint32_t hist[258];
  const int q = blockIdx.x;
  if (!qbig[q]) return;
  const uint32_t c = min(cnt[q], (uint32_t)CAP);
  float nt = -INFINITY;
  if (c >= (uint32_t)k) nt = wg_kth_largest(&surv[(size_t)q * CAP].score, c, 2, k, hist);
  __syncthreads();
  if (threadIdx.x == 0) {
    tau[q] = nt;
    cnt[q] = 0;
  }
}

}  // namespace

struct gann_index : IvfBase {
  // the lists' payload, and per group its segments
  Buf lf, lbias, nseg;
  bool any_big = false;  // some group holds more than CAP rows: round 0 opens with the sample pass
  // per-call scratch
  Buf qf, qss, qgroup, qbig, pstart, ntile, tstart, nwork, wstart, totals, work;
  // the last search
  int64_t last_tiles = 0, last_work = 0;
};

namespace {

int check_build(int32_t metric, int32_t d, int32_t n_groups, int64_t n) {
  if (metric < GANN_METRIC_L2 || metric > GANN_METRIC_INNER_PRODUCT) return fail(GANN_EINVAL, "unknown metric");
  if (d < 16 || d > MAX_D || d % 16) return fail(GANN_EINVAL, "dimension must be a multiple of 16 in 16..512");
  if (n_groups < 1 || n_groups > MAX_GROUPS) return fail(GANN_EINVAL, "n_groups must be in 1..1048576");
  if (n < 0 || n >= ((int64_t)1 << 31) - 64) return fail(GANN_EINVAL, "vector count out of range");
  return GANN_OK;
}

int search_chunk(gann_index *ix, int32_t nq, const float *queries, const int32_t *query_groups, int32_t k, float *out_dist,
                 int64_t *out_ids, int32_t *out_counts) {
  const int d = ix->d, S = d >> 4, ng = ix->nlist;
  hipStream_t st = 0;
  const int nq_pad = (nq + 31) / 32 * 32;
  ITRY(ix->stage.reserve((size_t)nq * d * sizeof(float)));
  ITRY(ix->qf.reserve((size_t)nq_pad * d * sizeof(_Float16) * 2));  // the fp16 rows, then the scan's fragments
  ITRY(ix->qsumsq.reserve((size_t)nq_pad * sizeof(float)));
  ITRY(ix->qss.reserve((size_t)nq_pad * sizeof(float)));
  ITRY(ix->qgroup.reserve((size_t)nq * 4));
  ITRY(ix->qbig.reserve((size_t)nq * 4));
  ITRY(ix->pair_cell.reserve((size_t)nq * 4));
  ITRY(ix->pair_q.reserve((size_t)nq * 4));
  ITRY(ix->pair_cell_s.reserve((size_t)nq * 4));
  ITRY(ix->pair_q_s.reserve((size_t)nq * 4));
  for (Buf *b : {&ix->per_cell, &ix->pstart, &ix->ntile, &ix->tstart, &ix->nwork, &ix->wstart}) ITRY(b->reserve((size_t)ng * 4));
  ITRY(ix->totals.reserve(8));
  ITRY(ix->rows_acc.reserve(8));
  ITRY(ix->tau.reserve((size_t)nq * 4));
  ITRY(ix->cnt.reserve((size_t)nq * 4));
  ITRY(ix->done_cnt.reserve((size_t)nq * 4));
  ITRY(ix->flags.reserve(sizeof(int)));
  ITRY(ix->surv.reserve((size_t)nq * CAP * sizeof(Survivor)));
  ITRY(ix->o_dist.reserve((size_t)nq * k * sizeof(float)));
  ITRY(ix->o_ids.reserve((size_t)nq * k * sizeof(int64_t)));
  ITRY(ix->o_cnt.reserve((size_t)nq * sizeof(int32_t)));
  _Float16 *q16 = ix->qf.as<_Float16>(), *qfrag = q16 + (size_t)nq_pad * d;

  // the queries as the scan's B fragments
  ITRY(hipEventRecord(ix->ev[0], st));
  ITRY(hipMemcpyAsync(ix->stage.p, queries, (size_t)nq * d * sizeof(float), hipMemcpyHostToDevice, st));
  ITRY(hipMemcpyAsync(ix->qgroup.p, query_groups, (size_t)nq * 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(store_rows_kernel, dim3(blocks_for(nq, 4)), dim3(256), 0, st, ix->stage.as<float>(), (int64_t)nq, d,
                     ix->metric == IVF_METRIC_COSINE ? 1 : 0, q16, ix->qss.as<float>());
  ITRY(hipGetLastError());
  hipLaunchKernelGGL(frag_rows_kernel, dim3(blocks_for((int64_t)nq * (d >> 3))), dim3(256), 0, st, q16, ix->qss.as<float>(), nq, d, S,
                     qfrag, ix->qsumsq.as<float>(), (_Float16 *)nullptr);
  ITRY(hipGetLastError());

  // (group, query) pairs sorted by group, tiles and work items
  ITRY(hipMemsetAsync(ix->per_cell.p, 0, (size_t)ng * 4, st));
  ITRY(hipMemsetAsync(ix->rows_acc.p, 0, 8, st));
  hipLaunchKernelGGL(pairs_kernel, dim3(blocks_for(nq)), dim3(256), 0, st, ix->qgroup.as<int32_t>(), nq, ng, ix->sizes.as<uint32_t>(),
                     ix->pair_cell.as<uint32_t>(), ix->pair_q.as<uint32_t>(), ix->per_cell.as<uint32_t>(), ix->qbig.as<uint32_t>(),
                     ix->rows_acc.as<unsigned long long>());
  ITRY(hipGetLastError());
  if (int rc = sort_by_cell(ix, ix->pair_cell.as<uint32_t>(), ix->pair_cell_s.as<uint32_t>(), ix->pair_q.as<uint32_t>(),
                            ix->pair_q_s.as<uint32_t>(), nq))
    return rc;
  hipLaunchKernelGGL(tiles_kernel, dim3(blocks_for(ng)), dim3(256), 0, st, ix->per_cell.as<uint32_t>(), ix->nseg.as<uint32_t>(), ng,
                     ix->ntile.as<uint32_t>(), ix->nwork.as<uint32_t>());
  ITRY(hipGetLastError());
  if (int rc = exclusive_sum(ix, ix->per_cell.as<uint32_t>(), ix->pstart.as<uint32_t>(), ng)) return rc;
  if (int rc = exclusive_sum(ix, ix->ntile.as<uint32_t>(), ix->tstart.as<uint32_t>(), ng)) return rc;
  if (int rc = exclusive_sum(ix, ix->nwork.as<uint32_t>(), ix->wstart.as<uint32_t>(), ng)) return rc;
  hipLaunchKernelGGL(totals_kernel, dim3(1), dim3(64), 0, st, ix->tstart.as<uint32_t>(), ix->ntile.as<uint32_t>(),
                     ix->wstart.as<uint32_t>(), ix->nwork.as<uint32_t>(), ng, ix->totals.as<uint32_t>());
  ITRY(hipGetLastError());
  uint32_t totals[2] = {0, 0};
  ITRY(hipMemcpy(totals, ix->totals.p, 8, hipMemcpyDeviceToHost));
  const uint32_t n_work = totals[1];
  ITRY(ix->work.reserve((size_t)n_work * sizeof(Work)));
  if (n_work) {
    hipLaunchKernelGGL(work_kernel, dim3(blocks_for(n_work)), dim3(256), 0, st, n_work, ix->wstart.as<uint32_t>(), ix->ntile.as<uint32_t>(),
                       ix->per_cell.as<uint32_t>(), ix->pstart.as<uint32_t>(), ix->boff.as<uint32_t>(), ix->nblk.as<uint32_t>(),
                       ix->sizes.as<uint32_t>(), ng, ix->work.as<Work>());
    ITRY(hipGetLastError());
  }

  // scan rounds
  ScanArgs a;
  a.lf = ix->lf.as<_Float16>();
  a.lbias = ix->lbias.as<float>();
  a.qf = qfrag;
  a.work = ix->work.as<Work>();
  a.pair_q = ix->pair_q_s.as<uint32_t>();
  a.tau = ix->tau.as<float>();
  a.cnt = ix->cnt.as<uint32_t>();
  a.surv = ix->surv.as<Survivor>();
  a.S = S;
  a.sample_pass = 0;
  const size_t lds = (size_t)S * 64 * sizeof(half8);
  int rounds = 0;
  if (int rc = scan_rounds(ix, nq, k, [&](int round, hipStream_t s) -> int {
        if (n_work == 0) return IVF_OK;
        if (round == 0 && ix->any_big) {
          ScanArgs sa = a;
          sa.sample_pass = 1;
          hipLaunchKernelGGL(segment_scan_kernel, dim3(n_work), dim3(256), lds, s, sa);
          ITRY(hipGetLastError());
          hipLaunchKernelGGL(sample_threshold_kernel, dim3(nq), dim3(256), 0, s, ix->qbig.as<uint32_t>(), ix->tau.as<float>(),
                             ix->cnt.as<uint32_t>(), ix->surv.as<Survivor>(), k);
          ITRY(hipGetLastError());
        }
        hipLaunchKernelGGL(segment_scan_kernel, dim3(n_work), dim3(256), lds, s, a);
        ITRY(hipGetLastError());
        return IVF_OK;
      }, &rounds))
    return rc;

  hipLaunchKernelGGL(select_kernel, dim3(nq), dim3(512), SELECT_LDS, st, ix->surv.as<Survivor>(), ix->done_cnt.as<uint32_t>(),
                     ix->qsumsq.as<float>(), ix->lrank.as<uint32_t>(), ix->ids_sorted.as<int64_t>(), ix->metric, k,
                     ix->o_dist.as<float>(), ix->o_ids.as<int64_t>(), ix->o_cnt.as<int32_t>());
  ITRY(hipGetLastError());
  ix->last_tiles += totals[0];
  ix->last_work += n_work;
  return finish_chunk(ix, nq, k, rounds, out_dist, out_ids, out_counts);
}

}  // namespace

extern "C" {

const char *gann_last_error(void) { return g_err.c_str(); }

int gann_index_build(int32_t device, int32_t metric, int32_t d, int32_t n_groups, int64_t n, const float *vectors,
                     const int64_t *ids, const int32_t *groups, gann_index_t **out) try {
  if (!out) return fail(GANN_EINVAL, "null argument");
  if (int rc = check_build(metric, d, n_groups, n)) return rc;
  if (n > 0 && (!vectors || !groups)) return fail(GANN_EINVAL, "null argument");
  for (int64_t i = 0; i < n; ++i)
    if (groups[i] < 0 || groups[i] >= n_groups)
      return fail(GANN_EINVAL, "row " + std::to_string(i) + ": its group " + std::to_string(groups[i]) + " is outside [0, n_groups = " +
                                   std::to_string(n_groups) + ")");
  ITRY(hipSetDevice(device));
  std::unique_ptr<gann_index> ix(new gann_index);
  if (int rc = init_base(ix.get(), device, metric, d, n_groups)) return rc;
  ix->cell_bits = GROUP_BITS;
  ITRY(hipFuncSetAttribute((const void *)select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SELECT_LDS));
  ITRY(ix->nseg.reserve((size_t)n_groups * 4));
  if (n > 0) {
    // the rows in the order given: they go with this call, the lists keep the only copy
    Buf flat, sumsq;
    if (int rc = grow_rows(ix.get(), n)) return rc;
    ITRY(flat.reserve((size_t)n * d * sizeof(_Float16)));
    ITRY(sumsq.reserve((size_t)n * 4));
    if (int rc = upload_rows(ix.get(), vectors, false, n, flat.as<_Float16>(), sumsq.as<float>())) return rc;
    ITRY(hipMemcpy(ix->cell.p, groups, (size_t)n * 4, hipMemcpyHostToDevice));
    if (int rc = commit_add(ix.get(), n, ids)) return rc;
    gann_index *p = ix.get();
    if (int rc = layout_lists(p, 32, [p, d, &flat, &sumsq](size_t slots) -> int {
          ITRY(p->lf.reserve(slots * d * sizeof(_Float16)));
          ITRY(p->lbias.reserve(slots * sizeof(float)));
          ITRY(hipMemset(p->lf.p, 0, slots * d * sizeof(_Float16)));
          hipLaunchKernelGGL(fill_kernel, dim3(blocks_for((int64_t)slots)), dim3(256), 0, 0, p->lbias.as<float>(), (int64_t)slots, -INFINITY);
          ITRY(hipGetLastError());
          hipLaunchKernelGGL(scatter_rows_kernel, dim3(blocks_for(p->n, 4)), dim3(256), 0, 0, flat.as<_Float16>(), sumsq.as<float>(), p->n,
                             d, p->metric, p->cell_sorted.as<uint32_t>(), p->ord.as<uint32_t>(), p->perm.as<uint32_t>(),
                             p->start.as<uint32_t>(), p->boff.as<uint32_t>(), p->lf.as<_Float16>(), p->lbias.as<float>(),
                             p->lrank.as<uint32_t>());
          ITRY(hipGetLastError());
          return IVF_OK;
        }))
      return rc;
  }
  hipLaunchKernelGGL(segments_kernel, dim3(blocks_for(n_groups)), dim3(256), 0, 0, ix->nblk.as<uint32_t>(), n_groups, ix->nseg.as<uint32_t>());
  ITRY(hipGetLastError());
  ITRY(hipDeviceSynchronize());
  // what only the layout needed: the index is immutable, a search reads the lists, lrank, ids_sorted and the per-group tables
  for (Buf *b : {&ix->stage, &ix->cell, &ix->ids, &ix->perm, &ix->cell_r, &ix->cell_sorted, &ix->ord, &ix->iota, &ix->sort_tmp}) b->release();
  ix->any_big = *std::max_element(ix->h_sizes.begin(), ix->h_sizes.end()) > CAP;
  *out = ix.release();
  return GANN_OK;
} ABI_CATCH

int gann_search(gann_index_t *ix, int32_t nq, const float *queries, const int32_t *query_groups, int32_t k, float *out_dist,
                int64_t *out_ids, int32_t *out_counts) try {
  if (!ix || !queries || !query_groups || !out_dist || !out_ids || !out_counts) return fail(GANN_EINVAL, "null argument");
  if (nq < 1) return fail(GANN_EINVAL, "nq must be positive");
  if (k < 1 || k > MAX_K) return fail(GANN_EINVAL, "k must be in 1..1024");
  ITRY(hipSetDevice(ix->device));
  ix->last_nq = 0;
  ix->last_rows = 0;
  ix->last_rounds = 0;
  ix->last_tiles = ix->last_work = 0;
  ix->t_coarse = ix->t_scan = ix->t_sel = 0;
  return search_chunks(ix, nq, [&](int32_t q0, int32_t m) -> int {
    return search_chunk(ix, m, queries + (size_t)q0 * ix->d, query_groups + q0, k, out_dist + (size_t)q0 * k, out_ids + (size_t)q0 * k,
                        out_counts + q0);
  });
} ABI_CATCH

int gann_index_info(const gann_index_t *ix, int64_t *n, int32_t *d, int32_t *metric, int32_t *n_groups) try {
  return index_info(ix, n, d, metric, n_groups);
} ABI_CATCH

int gann_index_group_sizes(const gann_index_t *ix, int64_t *out) try { return list_sizes(ix, out); } ABI_CATCH

int gann_last_stats(const gann_index_t *ix, int64_t *tiles, int64_t *work_items, int32_t *rounds, int64_t *rows_scanned,
                    int32_t *segment_rows, float *worklist_ms, float *scan_ms, float *select_ms) try {
  if (!ix) return fail(GANN_EINVAL, "null index");
  if (tiles) *tiles = ix->last_tiles;
  if (work_items) *work_items = ix->last_work;
  if (segment_rows) *segment_rows = SEG_ROWS;
  return last_stats(ix, rows_scanned, rounds, worklist_ms, scan_ms, select_ms);
} ABI_CATCH

int gann_index_destroy(gann_index_t *ix) try {
  delete ix;
  return GANN_OK;
} ABI_CATCH

}  // extern "C"
