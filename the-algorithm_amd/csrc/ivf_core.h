// ivf_core.h -- the host side that the two inverted-file indexes (ivf_ann.hip: flat lists; ivfpq_ann.hip: product-quantised
// lists) share, written once against IvfBase, the fields both index structs hold: row preparation and assignment, the
// layout of the lists up to the payload scatter, the steps of a search around the scan launch, the select step's key load
// (the sort itself is survivor_topk.h's), the steps of an add and of a restore around the payload, and the exports.  Where
// the two indexes differ the difference is an argument: the rows of a list block, a payload buffer and its row bytes, or a
// callable (the payload scatter, the scan launch).  The coarse step -- assign_rows and the first half of probe_chunk -- is
// the exhaustive search over the centroids, or, with an HNSW quantizer attached (ivf_hnsw_quantizer_internal.h), the walk
// of a graph over them.  Failures go through the error channel of ivf_error.h (host_error.h with
// the IVF_* codes).  A source includes this once, as it does ivf_kernels.h;
// everything is file-local.  Its host functions instantiate the hipcub sorts and scans, so only the index sources include
// it (the two above and grouped_ann.hip, whose cell is the caller's group: IvfBase without a coarse quantizer, cell_bits
// wide enough for its group numbers): opq_ann.hip and refine_ann.hip take ivf_error.h and ivf_kernels.h alone.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/dense_ann.h"
#include "../../include/hnsw_ann.h"
#include "../../include/ivf_ann.h"
#include "ann_by_id_internal.h"
#include "ivf_error.h"
#include "ivf_hnsw_quantizer_internal.h"
#include "ivf_kernels.h"
#include "ivf_restore.h"

namespace {

// a call into dense_ann.hip: its status codes carry the same numbers, its message is in dann_last_error()
#define DCALL(expr)                                              \
  do {                                                           \
    int rc_ = (expr);                                            \
    if (rc_) return fail(rc_, std::string("coarse quantizer: ") + dann_last_error()); \
  } while (0)
// a call into hnsw_ann.hip (the HNSW coarse quantizer): the same numbers again, its message is in hnsw_last_error()
#define HQCALL(expr)                                             \
  do {                                                           \
    int rc_ = (expr);                                            \
    if (rc_) return fail(rc_, std::string("HNSW coarse quantizer: ") + hnsw_last_error()); \
  } while (0)

// what an ivf_index and an ivfpq_index both hold; each adds its payload (rows or codes), its list payload and its own scratch
struct IvfBase {
  int device = 0, metric = 0, d = 0, nlist = 0;
  int cell_bits = CELL_BITS;  // radix-sort key width of a cell number of this index
  int64_t n = 0;
  int ids_mode = -1;  // -1: no add yet; 0: ids are positions; 1: ids given
  dann_index *coarse = nullptr;
  ivf_hq::State hq;  // the optional HNSW coarse quantizer (ivf_hnsw_quantizer_internal.h); hq.graph is owned
  Buf hq_lastq, hq_missing;  // the prepared queries of the last search that walked; the missing probes of a chunk
  // per row, in the order added
  Buf cell, ids;
  // the lists: every list starts on a block of `lblock` rows (layout_lists); lrank[slot] is the slot's rank in id order
  Buf ids_sorted, perm, cell_r, cell_sorted, ord, iota, sizes, start, nblk, boff, lrank, sort_tmp;
  std::vector<int64_t> h_sizes;
  int64_t total_blocks = 0;
  // per-call scratch
  Buf stage, c_dist, c_ids, c_cnt, qsumsq;
  Buf pair_cell, pair_q, pair_cell_s, pair_q_s, per_cell, rows_acc;
  Buf tau, cnt, done_cnt, surv, flags, o_dist, o_ids, o_cnt;
  // the last search
  Buf probes;
  int32_t last_nq = 0, last_nprobe = 0, last_rounds = 0;
  int64_t last_rows = 0;
  int64_t chunk_pairs = 0;  // the (cell, query) pairs of the last chunk that name a cell: all of them, but for a short walk
  int64_t last_ctl = 0;  // control bytes the search read back: round flags, row and group counts (never an answer)
  int64_t last_ctl_up = 0;  // the part of last_ctl that went up instead: an HNSW quantizer's second-pass query list
  std::shared_ptr<void> by_id;  // the by-id scratch of this index (faiss_by_id.hip), freed with it
  float t_coarse = 0, t_scan = 0, t_sel = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  RestoreState rs;  // faiss_restore.h
  ~IvfBase() {
    if (coarse) (void)dann_index_destroy(coarse);
    if (hq.graph) (void)hnsw_index_destroy(hq.graph);
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

constexpr size_t SELECT_LDS = CAP * sizeof(unsigned long long);  // the select kernels' dynamic LDS: one key per survivor

int check_shape(int32_t metric, int32_t d, int32_t nlist) {
  if (metric < IVF_METRIC_L2 || metric > IVF_METRIC_INNER_PRODUCT) return fail(IVF_EINVAL, "unknown metric");
  if (d < 16 || d > MAX_D || d % 16) return fail(IVF_EINVAL, "dimension must be a multiple of 16 in 16..512");
  if (nlist < 1 || nlist > MAX_NLIST) return fail(IVF_EINVAL, "nlist must be in 1..65536");
  return IVF_OK;
}

// the shared fields of a new, empty index (the device is current)
int init_base(IvfBase *ix, int32_t device, int32_t metric, int32_t d, int32_t nlist) {
  ix->device = device;
  ix->metric = metric;
  ix->d = d;
  ix->nlist = nlist;
  ix->h_sizes.assign((size_t)nlist, 0);
  for (auto &e : ix->ev) ITRY(hipEventCreate(&e));
  for (Buf *b : {&ix->sizes, &ix->start, &ix->nblk, &ix->boff}) {
    ITRY(b->reserve((size_t)nlist * 4));
    ITRY(hipMemset(b->p, 0, (size_t)nlist * 4));
  }
  return IVF_OK;
}

// ---------------------------------------------------------------------------------------------
// rows -> fp16 rows, and their cells
// ---------------------------------------------------------------------------------------------
inline int64_t stage_slab_rows(int d) { return std::max<int64_t>(1, (int64_t)(64 << 20) / (d * 4)); }
// host rows -> the staging buffer of the index
int stage_rows(IvfBase *ix, const float *rows, int64_t m) {
  ITRY(ix->stage.reserve((size_t)m * ix->d * sizeof(float)));
  ITRY(hipMemcpy(ix->stage.p, rows, (size_t)m * ix->d * sizeof(float), hipMemcpyHostToDevice));
  return IVF_OK;
}
// m device rows -> fp16 rows at `flat` and their sums of squares at `sumsq`
int prepare_slab(IvfBase *ix, const float *d_rows, int64_t m, _Float16 *flat, float *sumsq) {
  hipLaunchKernelGGL(store_rows_kernel, dim3(blocks_for(m, 4)), dim3(256), 0, 0, d_rows, m, ix->d,
                     ix->metric == IVF_METRIC_COSINE ? 1 : 0, flat, sumsq);
  ITRY(hipGetLastError());
  ITRY(hipDeviceSynchronize());
  return IVF_OK;
}
// n rows, on the host or on the device (ivf_device_rows.h), prepared a slab at a time
int upload_rows(IvfBase *ix, const float *rows, bool on_device, int64_t n, _Float16 *flat, float *sumsq) {
  const int64_t slab = stage_slab_rows(ix->d);
  for (int64_t r0 = 0; r0 < n; r0 += slab) {
    const int64_t m = std::min(slab, n - r0);
    const float *src = rows + r0 * ix->d;
    if (!on_device) {
      if (int rc = stage_rows(ix, src, m)) return rc;
      src = ix->stage.as<float>();
    }
    if (int rc = prepare_slab(ix, src, m, flat + (size_t)r0 * ix->d, sumsq + r0)) return rc;
  }
  return IVF_OK;
}

// stable sort of n (cell number, value) pairs by cell
int sort_by_cell(IvfBase *ix, const uint32_t *keys, uint32_t *keys_out, const uint32_t *vals, uint32_t *vals_out, int64_t n) {
  size_t tb = 0;
  ITRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys, keys_out, vals, vals_out, (int)n, 0, ix->cell_bits, (hipStream_t)0));
  ITRY(ix->sort_tmp.reserve(tb));
  ITRY(hipcub::DeviceRadixSort::SortPairs(ix->sort_tmp.p, tb, keys, keys_out, vals, vals_out, (int)n, 0, ix->cell_bits, (hipStream_t)0));
  return IVF_OK;
}
int exclusive_sum(IvfBase *ix, const uint32_t *in, uint32_t *out, int n) {
  size_t tb = 0;
  ITRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, n, (hipStream_t)0));
  ITRY(ix->sort_tmp.reserve(tb));
  ITRY(hipcub::DeviceScan::ExclusiveSum(ix->sort_tmp.p, tb, in, out, n, (hipStream_t)0));
  return IVF_OK;
}

// the nearest centroid of each of n fp16 rows (the coarse search with k = 1, CHUNK rows at a time) -> cell[0 .. n)
// With an HNSW quantizer attached: the walk with k = 1 at the index's quantizer_ef, as Faiss's add goes through the quantizer.
int assign_rows_walk(IvfBase *ix, const _Float16 *flat, int64_t n, int32_t *cell) {
  const int d = ix->d, ef = ix->hq.ef;
  for (int64_t r0 = 0; r0 < n; r0 += CHUNK) {
    const int m = (int)std::min<int64_t>(CHUNK, n - r0);
    ann_by_id::HnswTarget tgt;
    HQCALL(ann_by_id::hnsw_open(ix->hq.graph, m, 1, ef, false, &tgt));
    hipLaunchKernelGGL(hq_rows_kernel, dim3(blocks_for((int64_t)m * (tgt.dpad >> 3))), dim3(256), 0, 0, flat + (size_t)r0 * d, m, d,
                       tgt.dpad, tgt.q);
    ITRY(hipGetLastError());
    ann_by_id::DeviceResult res;
    HQCALL(ann_by_id::hnsw_search_prepared(ix->hq.graph, m, 1, ef, &res));
    hipLaunchKernelGGL(cells_kernel, dim3(blocks_for(m)), dim3(256), 0, 0, res.ids, m, cell + r0);
    ITRY(hipGetLastError());
  }
  ITRY(hipDeviceSynchronize());
  return IVF_OK;
}
int assign_rows(IvfBase *ix, const _Float16 *flat, const float *sumsq, int64_t n, int32_t *cell) {
  if (ix->hq.graph) return assign_rows_walk(ix, flat, n, cell);
  ann_by_id::DannTarget tgt;
  DCALL(ann_by_id::dann_open(ix->coarse, 1, false, &tgt));
  ITRY(ix->c_dist.reserve((size_t)CHUNK * sizeof(float)));
  ITRY(ix->c_ids.reserve((size_t)CHUNK * sizeof(int64_t)));
  ITRY(ix->c_cnt.reserve((size_t)CHUNK * sizeof(int32_t)));
  const int d = ix->d;
  for (int64_t r0 = 0; r0 < n; r0 += CHUNK) {
    const int m = (int)std::min<int64_t>(CHUNK, n - r0);
    ann_by_id::DannChunk ch;
    DCALL(ann_by_id::dann_chunk_open(ix->coarse, m, 1, &ch));
    hipLaunchKernelGGL(frag_rows_kernel, dim3(blocks_for((int64_t)m * (d >> 3))), dim3(256), 0, 0, flat + (size_t)r0 * d,
                       sumsq + r0, m, d, tgt.S, ch.qf, ch.qsumsq, (_Float16 *)nullptr);
    ITRY(hipGetLastError());
    int64_t d2h = 0;
    DCALL(ann_by_id::dann_chunk_search_prepared(ix->coarse, m, 1, ix->c_dist.as<float>(), ix->c_ids.as<int64_t>(),
                                                ix->c_cnt.as<int32_t>(), &d2h));
    hipLaunchKernelGGL(cells_kernel, dim3(blocks_for(m)), dim3(256), 0, 0, ix->c_ids.as<int64_t>(), m, cell + r0);
    ITRY(hipGetLastError());
  }
  ITRY(hipDeviceSynchronize());
  return IVF_OK;
}

// ---------------------------------------------------------------------------------------------
// list construction
// ---------------------------------------------------------------------------------------------
// cells of n rows -> their order by (cell, position): ord, and per cell its size and first place in that order
int segment_by_cell(IvfBase *ix, const uint32_t *perm, int64_t n) {
  ITRY(ix->cell_r.reserve((size_t)n * 4));
  ITRY(ix->cell_sorted.reserve((size_t)n * 4));
  ITRY(ix->ord.reserve((size_t)n * 4));
  ITRY(ix->iota.reserve((size_t)n * 4));
  ITRY(hipMemset(ix->sizes.p, 0, (size_t)ix->nlist * 4));
  if (n > 0) {
    hipLaunchKernelGGL(gather_cells_kernel, dim3(blocks_for(n)), dim3(256), 0, 0, ix->cell.as<int32_t>(), perm, n,
                       ix->cell_r.as<uint32_t>());
    ITRY(hipGetLastError());
    hipLaunchKernelGGL(iota_kernel, dim3(blocks_for(n)), dim3(256), 0, 0, ix->iota.as<uint32_t>(), n);
    ITRY(hipGetLastError());
    if (int rc = sort_by_cell(ix, ix->cell_r.as<uint32_t>(), ix->cell_sorted.as<uint32_t>(), ix->iota.as<uint32_t>(),
                              ix->ord.as<uint32_t>(), n))
      return rc;
    hipLaunchKernelGGL(hist_kernel, dim3(blocks_for(n)), dim3(256), 0, 0, ix->cell_r.as<uint32_t>(), n, ix->sizes.as<uint32_t>());
    ITRY(hipGetLastError());
  }
  return exclusive_sum(ix, ix->sizes.as<uint32_t>(), ix->start.as<uint32_t>(), ix->nlist);
}

// all lists again from the rows in the order added: (cell, id) order, every list on a boundary of `lblock` rows.  The
// bookkeeping (ids_sorted, perm, cell_sorted, ord, sizes, start, nblk, boff, a zeroed lrank) is laid out here; then
// scatter(slots) sizes the index's own list payload and fills it and lrank.
template <class Scatter>
int layout_lists(IvfBase *ix, int lblock, Scatter scatter) {
  const int64_t n = ix->n;
  const int nlist = ix->nlist;
  // rank in (id, position) order: ids_sorted[rank], perm[rank] = position
  ITRY(ix->ids_sorted.reserve((size_t)n * 8));
  ITRY(ix->perm.reserve((size_t)n * 4));
  ITRY(ix->iota.reserve((size_t)n * 4));
  hipLaunchKernelGGL(iota_kernel, dim3(blocks_for(n)), dim3(256), 0, 0, ix->iota.as<uint32_t>(), n);
  ITRY(hipGetLastError());
  size_t tb = 0;
  ITRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const int64_t *)nullptr, (int64_t *)nullptr, (const uint32_t *)nullptr,
                                          (uint32_t *)nullptr, (int)n, 0, 64, (hipStream_t)0));
  ITRY(ix->sort_tmp.reserve(tb));
  ITRY(hipcub::DeviceRadixSort::SortPairs(ix->sort_tmp.p, tb, ix->ids.as<int64_t>(), ix->ids_sorted.as<int64_t>(),
                                          ix->iota.as<uint32_t>(), ix->perm.as<uint32_t>(), (int)n, 0, 64, (hipStream_t)0));
  ITRY(hipDeviceSynchronize());  // (the sorts below may replace sort_tmp)
  // ranks by (cell, rank)
  if (int rc = segment_by_cell(ix, ix->perm.as<uint32_t>(), n)) return rc;
  hipLaunchKernelGGL(blocks_of_kernel, dim3(blocks_for(nlist)), dim3(256), 0, 0, ix->sizes.as<uint32_t>(), nlist, (uint32_t)lblock,
                     ix->nblk.as<uint32_t>());
  ITRY(hipGetLastError());
  if (int rc = exclusive_sum(ix, ix->nblk.as<uint32_t>(), ix->boff.as<uint32_t>(), nlist)) return rc;
  std::vector<uint32_t> hs((size_t)nlist);
  ITRY(hipMemcpy(hs.data(), ix->sizes.p, (size_t)nlist * 4, hipMemcpyDeviceToHost));
  int64_t blocks = 0;
  for (int c = 0; c < nlist; ++c) {
    ix->h_sizes[(size_t)c] = hs[(size_t)c];
    blocks += (hs[(size_t)c] + lblock - 1) / lblock;
  }
  if (blocks * lblock >= (int64_t)0xffffff00u) return fail(IVF_ELIMIT, "the lists would hold 2^32 slots or more");
  ix->total_blocks = blocks;
  const size_t slots = (size_t)blocks * lblock;
  ITRY(ix->lrank.reserve(slots * sizeof(uint32_t)));
  ITRY(hipMemset(ix->lrank.p, 0, slots * sizeof(uint32_t)));
  if (int rc = scatter(slots)) return rc;
  ITRY(hipDeviceSynchronize());
  return IVF_OK;
}

// ---------------------------------------------------------------------------------------------
// a search: search_begin, then per chunk of <= CHUNK queries (search_chunks) probe_chunk, the index's own group table
// or pair grid, scan_rounds over its scan launch, its select launch, finish_chunk
// ---------------------------------------------------------------------------------------------
// the checks and resets of a search; nprobe comes back clamped to nlist
int search_begin(IvfBase *ix, int32_t nq, int32_t k, int32_t *nprobe) {
  if (nq < 1) return fail(IVF_EINVAL, "nq must be positive");
  if (k < 1 || k > MAX_K) return fail(IVF_EINVAL, "k must be in 1..1024");
  if (*nprobe < 1 || *nprobe > MAX_NPROBE) return fail(IVF_EINVAL, "nprobe must be in 1..1024");
  *nprobe = std::min(*nprobe, ix->nlist);
  ITRY(hipSetDevice(ix->device));
  ITRY(ix->probes.reserve((size_t)nq * *nprobe * sizeof(int32_t)));
  ix->last_nq = 0;
  ix->last_nprobe = *nprobe;
  ix->last_rows = 0;
  ix->last_rounds = 0;
  ix->last_ctl = ix->last_ctl_up = 0;
  ix->t_coarse = ix->t_scan = ix->t_sel = 0;
  ix->hq.evals = ix->hq.expansions = ix->hq.missing = 0;
  ix->hq.last_q_n = 0;
  if (ix->hq.graph) {
    ITRY(ix->hq_lastq.reserve((size_t)nq * ix->d * sizeof(_Float16)));
    ITRY(ix->hq_missing.reserve(sizeof(uint32_t)));
    ix->hq.last_q = ix->hq_lastq.p;
  }
  return IVF_OK;
}
// chunk(q0, m) over the queries, CHUNK at a time
template <class Chunk>
int search_chunks(IvfBase *ix, int32_t nq, Chunk chunk) {
  for (int32_t q0 = 0; q0 < nq; q0 += CHUNK)
    if (int rc = chunk(q0, std::min<int32_t>(CHUNK, nq - q0))) return rc;
  ix->last_nq = nq;
  if (ix->hq.graph) ix->hq.last_q_n = nq;
  return IVF_OK;
}

// With an HNSW quantizer attached (ix->hq.graph) the coarse search is the graph's walk with k = nprobe at quantizer_ef, and
// a probe the walk did not find is exported as -1 and scanned by nobody (hq_probes_kernel); chunk_pairs counts the rest.
// The first step of a chunk, from event 0: the queries (on the host, or on the device already) -> fp16 rows at q16 and,
// with qfrag != NULL, the fragments of the flat scan; the coarse search for their nprobe nearest centroids; the probe
// export; the (cell, query) pairs sorted by cell (pair_cell_s, pair_q_s) and the queries per cell (per_cell).  rows_acc is
// zeroed for the caller's count of the rows scanned.
// The queries come from one of three places: nq host rows at `queries`; nq device rows there (on_device); or, with pos !=
// NULL, rows of a device-resident store read through a position list (a by-id query, include/faiss_by_id.h): `queries` is
// the store's first row and query i is its row pos[i], prepared by store_rows_pos_kernel with no fp32 copy in between.
int probe_chunk(IvfBase *ix, int32_t q0, int32_t nq, const float *queries, bool on_device, const int64_t *pos, int32_t k,
                int32_t nprobe, _Float16 *q16, _Float16 *qfrag) {
  const int d = ix->d, nlist = ix->nlist;
  const int64_t np = (int64_t)nq * nprobe;
  hipStream_t st = 0;
  const bool walk = ix->hq.graph != nullptr;  // the HNSW quantizer: the graph is walked, the centroids are not scanned
  ann_by_id::DannTarget tgt;
  ann_by_id::DannChunk ch;
  if (!walk || qfrag) {  // (the flat scan's fragments are written beside the exhaustive search's)
    DCALL(ann_by_id::dann_open(ix->coarse, nprobe, false, &tgt));
    DCALL(ann_by_id::dann_chunk_open(ix->coarse, nq, nprobe, &ch));
  }
  ann_by_id::HnswTarget wt;
  if (walk) HQCALL(ann_by_id::hnsw_open(ix->hq.graph, nq, nprobe, ix->hq.ef, false, &wt));
  if (!on_device) ITRY(ix->stage.reserve((size_t)nq * d * sizeof(float)));
  ITRY(ix->qsumsq.reserve((size_t)((nq + 31) / 32 * 32) * sizeof(float)));
  ITRY(ix->c_dist.reserve((size_t)np * sizeof(float)));
  ITRY(ix->c_ids.reserve((size_t)np * sizeof(int64_t)));
  ITRY(ix->c_cnt.reserve((size_t)std::max(nq, CHUNK) * sizeof(int32_t)));
  ITRY(ix->pair_cell.reserve((size_t)np * 4));
  ITRY(ix->pair_q.reserve((size_t)np * 4));
  ITRY(ix->pair_cell_s.reserve((size_t)np * 4));
  ITRY(ix->pair_q_s.reserve((size_t)np * 4));
  ITRY(ix->per_cell.reserve((size_t)nlist * 4));
  ITRY(ix->rows_acc.reserve(8));
  ITRY(ix->tau.reserve((size_t)nq * 4));
  ITRY(ix->cnt.reserve((size_t)nq * 4));
  ITRY(ix->done_cnt.reserve((size_t)nq * 4));
  ITRY(ix->flags.reserve(sizeof(int)));
  ITRY(ix->surv.reserve((size_t)nq * CAP * sizeof(Survivor)));
  ITRY(ix->o_dist.reserve((size_t)nq * k * sizeof(float)));
  ITRY(ix->o_ids.reserve((size_t)nq * k * sizeof(int64_t)));
  ITRY(ix->o_cnt.reserve((size_t)nq * sizeof(int32_t)));

  // coarse: the nprobe nearest centroids of every query
  ITRY(hipEventRecord(ix->ev[0], st));
  if (!on_device) ITRY(hipMemcpyAsync(ix->stage.p, queries, (size_t)nq * d * sizeof(float), hipMemcpyHostToDevice, st));
  if (pos) {
    hipLaunchKernelGGL(store_rows_pos_kernel, dim3(blocks_for(nq, 4)), dim3(256), 0, st, queries, pos, (int64_t)nq, d,
                       ix->metric == IVF_METRIC_COSINE ? 1 : 0, q16, ix->qsumsq.as<float>());
  } else {
    hipLaunchKernelGGL(store_rows_kernel, dim3(blocks_for(nq, 4)), dim3(256), 0, st, on_device ? queries : ix->stage.as<float>(),
                       (int64_t)nq, d, ix->metric == IVF_METRIC_COSINE ? 1 : 0, q16, ix->qsumsq.as<float>());
  }
  ITRY(hipGetLastError());
  if (!walk || qfrag) {
    hipLaunchKernelGGL(frag_rows_kernel, dim3(blocks_for((int64_t)nq * (d >> 3))), dim3(256), 0, st, q16, ix->qsumsq.as<float>(), nq, d,
                       tgt.S, ch.qf, ch.qsumsq, qfrag);
    ITRY(hipGetLastError());
  }
  ix->chunk_pairs = np;
  if (walk) {
    // the walk for the nprobe nearest cells of every query, answers left on the device; a walk may find fewer
    hipLaunchKernelGGL(hq_rows_kernel, dim3(blocks_for((int64_t)nq * (wt.dpad >> 3))), dim3(256), 0, st, q16, nq, d, wt.dpad, wt.q);
    ITRY(hipGetLastError());
    ITRY(hipMemcpyAsync(ix->hq_lastq.as<_Float16>() + (size_t)q0 * d, q16, (size_t)nq * d * sizeof(_Float16), hipMemcpyDeviceToDevice, st));
    ann_by_id::DeviceResult res;
    HQCALL(ann_by_id::hnsw_search_prepared(ix->hq.graph, nq, nprobe, ix->hq.ef, &res));
    ix->last_ctl += res.h2d_bytes + res.d2h_bytes;
    ix->last_ctl_up += res.h2d_bytes;
    int64_t evals = 0, expansions = 0;
    HQCALL(hnsw_last_stats(ix->hq.graph, &evals, &expansions, nullptr, nullptr));
    ix->hq.evals += evals;
    ix->hq.expansions += expansions;
    ITRY(hipMemsetAsync(ix->per_cell.p, 0, (size_t)nlist * 4, st));
    ITRY(hipMemsetAsync(ix->rows_acc.p, 0, 8, st));
    ITRY(hipMemsetAsync(ix->hq_missing.p, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(hq_probes_kernel, dim3(blocks_for(np)), dim3(256), 0, st, res.ids, res.counts, nq, nprobe,
                       ix->probes.as<int32_t>() + (size_t)q0 * nprobe, ix->pair_cell.as<uint32_t>(), ix->pair_q.as<uint32_t>(),
                       ix->per_cell.as<uint32_t>(), ix->hq_missing.as<uint32_t>());
    ITRY(hipGetLastError());
    uint32_t missing = 0;
    ITRY(hipMemcpyAsync(&missing, ix->hq_missing.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    ITRY(hipStreamSynchronize(st));
    ix->last_ctl += (int64_t)sizeof(uint32_t);
    ix->hq.missing += missing;
    ix->chunk_pairs = np - (int64_t)missing;  // the pairs of the missing probes sort behind these
  } else {
    int64_t d2h = 0;
    DCALL(ann_by_id::dann_chunk_search_prepared(ix->coarse, nq, nprobe, ix->c_dist.as<float>(), ix->c_ids.as<int64_t>(),
                                                ix->c_cnt.as<int32_t>(), &d2h));
    ix->last_ctl += d2h;

    // inversion: (cell, query) pairs sorted by cell
    ITRY(hipMemsetAsync(ix->per_cell.p, 0, (size_t)nlist * 4, st));
    ITRY(hipMemsetAsync(ix->rows_acc.p, 0, 8, st));
    hipLaunchKernelGGL(probes_kernel, dim3(blocks_for(np)), dim3(256), 0, st, ix->c_ids.as<int64_t>(), nq, nprobe,
                       ix->probes.as<int32_t>() + (size_t)q0 * nprobe, ix->pair_cell.as<uint32_t>(), ix->pair_q.as<uint32_t>(),
                       ix->per_cell.as<uint32_t>());
    ITRY(hipGetLastError());
  }
  return sort_by_cell(ix, ix->pair_cell.as<uint32_t>(), ix->pair_cell_s.as<uint32_t>(), ix->pair_q.as<uint32_t>(),
                      ix->pair_q_s.as<uint32_t>(), np);
}

// Arms the survivor buffers (event 1), then the rounds of threshold refinement up to event 2: launch(round, stream) runs the
// index's scan, refine_kernel finishes or re-arms every query.  *rounds = the fallback rounds taken.
template <class Launch>
int scan_rounds(IvfBase *ix, int32_t nq, int32_t k, Launch launch, int *rounds) {
  hipStream_t st = 0;
  hipLaunchKernelGGL(arm_kernel, dim3(blocks_for(nq)), dim3(256), 0, st, ix->tau.as<float>(), ix->cnt.as<uint32_t>(),
                     ix->done_cnt.as<uint32_t>(), nq);
  ITRY(hipGetLastError());
  ITRY(hipEventRecord(ix->ev[1], st));
  for (*rounds = 0;; ++*rounds) {
    if (int rc = launch(*rounds, st)) return rc;
    int flags = 0;
    ITRY(hipMemsetAsync(ix->flags.p, 0, sizeof(int), st));
    hipLaunchKernelGGL(refine_kernel, dim3(nq), dim3(256), 0, st, ix->tau.as<float>(), ix->cnt.as<uint32_t>(),
                       ix->done_cnt.as<uint32_t>(), ix->surv.as<Survivor>(), k, ix->flags.as<int>());
    ITRY(hipGetLastError());
    ITRY(hipMemcpyAsync(&flags, ix->flags.p, sizeof(int), hipMemcpyDeviceToHost, st));
    ITRY(hipStreamSynchronize(st));
    ix->last_ctl += (int64_t)sizeof(int);
    if (flags & 2) return fail(IVF_ELIMIT, "more than 8192 rows of the probed lists tie at the k-th distance of a query");
    if (*rounds >= 16) return fail(IVF_ELIMIT, "threshold refinement did not converge");
    if (!(flags & 1)) break;
  }
  ITRY(hipEventRecord(ix->ev[2], st));
  return IVF_OK;
}

// The last step of a chunk, after the select launch (event 3): with out_dist != NULL the answers of o_dist / o_ids / o_cnt
// go to the host (a search whose answer stays on the device -- ivf_device_rows.h's search_device_out -- passes NULL: its
// select launch wrote to the caller's device buffers); the rows scanned and the three phase times are added to the stats of the search.
int finish_chunk(IvfBase *ix, int32_t nq, int32_t k, int rounds, float *out_dist, int64_t *out_ids, int32_t *out_counts) {
  hipStream_t st = 0;
  ITRY(hipEventRecord(ix->ev[3], st));
  if (out_dist) {
    ITRY(hipMemcpyAsync(out_dist, ix->o_dist.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
    ITRY(hipMemcpyAsync(out_ids, ix->o_ids.p, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ITRY(hipMemcpyAsync(out_counts, ix->o_cnt.p, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  }
  unsigned long long rows = 0;
  ITRY(hipMemcpyAsync(&rows, ix->rows_acc.p, 8, hipMemcpyDeviceToHost, st));
  ITRY(hipStreamSynchronize(st));
  float tc = 0, ts = 0, tl = 0;
  (void)hipEventElapsedTime(&tc, ix->ev[0], ix->ev[1]);
  (void)hipEventElapsedTime(&ts, ix->ev[1], ix->ev[2]);
  (void)hipEventElapsedTime(&tl, ix->ev[2], ix->ev[3]);
  ix->t_coarse += tc;
  ix->t_scan += ts;
  ix->t_sel += tl;
  ix->last_rows += (int64_t)rows;
  ix->last_ctl += 8;
  ix->last_rounds = std::max(ix->last_rounds, rounds + 1);
  return IVF_OK;
}

// The select step of query q, one workgroup: its survivors as keys (score desc, rank in id order asc) in `keys`, sorted by
// survivor_topk.h's network, the one dense_ann.hip's select runs.  Returns the number of survivors; keys[i] >> 32 is f2key
// of the i-th best score, 0xffffffff - (uint32_t)keys[i] its rank.
__device__ __forceinline__ uint32_t select_sorted(const Survivor *__restrict__ surv, const uint32_t *__restrict__ done_cnt,
                                                  const uint32_t *__restrict__ lrank, int q, unsigned long long *keys) {
  const uint32_t c = min(done_cnt[q], (uint32_t)CAP);
  uint32_t n2 = 64;
  while (n2 < c) n2 <<= 1;
  for (uint32_t i = threadIdx.x; i < n2; i += blockDim.x) {
    unsigned long long key = 0;
    if (i < c) {
      Survivor s = surv[(size_t)q * CAP + i];
      key = ((unsigned long long)f2key(s.score) << 32) | (0xffffffffu - lrank[s.pos]);
    }
    keys[i] = key;
  }
  __syncthreads();
  sort_keys_desc(keys, n2);
  return c;
}

// ---------------------------------------------------------------------------------------------
// an add: the ids rule, room for the rows, then (the payload being in) the ids and the commit; the caller lays out
// ---------------------------------------------------------------------------------------------
int check_ids_rule(const IvfBase *ix, bool with_ids) {
  if (ix->ids_mode == 1 && !with_ids) return fail(IVF_EINVAL, "the index holds rows added with ids: an add must give ids");
  if (ix->ids_mode == 0 && with_ids) return fail(IVF_EINVAL, "the index holds rows added without ids (its ids are positions): ids must be NULL");
  return IVF_OK;
}
// room for n more cells and ids, the rows there are kept; makes the device current
int grow_rows(IvfBase *ix, int64_t n) {
  const int64_t n_old = ix->n, total = n_old + n;
  if (total >= ((int64_t)1 << 31) - 64) return fail(IVF_EINVAL, "vector count out of range");
  ITRY(hipSetDevice(ix->device));
  ITRY(ix->cell.grow_keep((size_t)n_old * 4, (size_t)total * 4));
  ITRY(ix->ids.grow_keep((size_t)n_old * 8, (size_t)total * 8));
  return IVF_OK;
}
int commit_add(IvfBase *ix, int64_t n, const int64_t *ids) {
  const int64_t n_old = ix->n;
  if (ids) {
    ITRY(hipMemcpy(ix->ids.as<int64_t>() + n_old, ids, (size_t)n * 8, hipMemcpyHostToDevice));
  } else {
    hipLaunchKernelGGL(iota64_kernel, dim3(blocks_for(n)), dim3(256), 0, 0, ix->ids.as<int64_t>() + n_old, n_old, n);
    ITRY(hipGetLastError());
  }
  ix->n = n_old + n;
  ix->ids_mode = ids ? 1 : 0;
  return IVF_OK;
}

// ---------------------------------------------------------------------------------------------
// restoring a saved index (faiss_restore.h): `payload` is the index's per-row column (rows or codes), row_bytes its row
// ---------------------------------------------------------------------------------------------
int check_restore(int32_t ids_mode, int64_t n) {
  if (n < 0 || n >= ((int64_t)1 << 31) - 64) return fail(IVF_EINVAL, "vector count out of range");
  if (ids_mode < -1 || ids_mode > 1 || (n == 0) != (ids_mode == -1)) return fail(IVF_EINVAL, "ids mode does not fit the row count");
  return IVF_OK;
}
// a new index with its coarse quantizer built expects n rows: their cells and ids get room, the restore is open
int restore_open(IvfBase *ix, int32_t ids_mode, int64_t n) {
  ITRY(ix->cell.reserve((size_t)n * 4));
  ITRY(ix->ids.reserve((size_t)n * 8));
  ix->rs.n = n;
  ix->rs.ids_mode = ids_mode;
  ix->rs.open = true;
  return IVF_OK;
}
int restore_staging(IvfBase *ix, int64_t m, int64_t max_rows, size_t row_bytes, int64_t **ids, int32_t **cells, void **payload) {
  if (!ix || !ix->rs.open || !ids || !cells || !payload) return fail(IVF_EINVAL, "no restore in progress");
  if (m < 1 || m > max_rows) return fail(IVF_EINVAL, "slab size out of range");
  ITRY(hipSetDevice(ix->device));
  ITRY(ix->rs.stage(m, row_bytes));
  *ids = ix->rs.ids();
  *cells = ix->rs.cells();
  *payload = ix->rs.payload();
  return IVF_OK;
}
// the staged slab -> rows [r0, r0 + m) of ids, cell and payload, validated; rs.done is the caller's to advance
int restore_rows(IvfBase *ix, int64_t r0, int64_t m, void *payload) {
  if (!ix || !ix->rs.open) return fail(IVF_EINVAL, "no restore in progress");
  RestoreState &rs = ix->rs;
  if (m < 1 || m > rs.slab || r0 != rs.done || m > rs.n - r0) return fail(IVF_EINVAL, "slab outside the rows announced");
  ITRY(hipSetDevice(ix->device));
  uint32_t bad[2] = {0, 0};
  ITRY(restore_upload(rs, r0, m, ix->nlist, ix->ids.as<int64_t>(), ix->cell.as<int32_t>(), payload, bad));
  if (bad[0] != 0xffffffffu)
    return fail(IVF_EINVAL, "row " + std::to_string(bad[0]) + ": its cell is outside [0, nlist = " + std::to_string(ix->nlist) + ")");
  if (bad[1] != 0xffffffffu)
    return fail(IVF_EINVAL, "row " + std::to_string(bad[1]) + ": the ids of this index are positions, and its id is not its position");
  return IVF_OK;
}
// every row is in: the index takes the count and the ids mode; the caller lays out if n > 0
int restore_close(IvfBase *ix) {
  if (!ix || !ix->rs.open) return fail(IVF_EINVAL, "no restore in progress");
  if (ix->rs.done != ix->rs.n) return fail(IVF_EINVAL, "rows are missing");
  ITRY(hipSetDevice(ix->device));
  ix->n = ix->rs.n;
  ix->ids_mode = ix->rs.ids_mode;
  ix->rs.close();
  return IVF_OK;
}
int export_columns(const IvfBase *ix, int64_t r0, int64_t m, int64_t *ids, int32_t *cells, void *out, const void *payload, size_t row_bytes) {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (r0 < 0 || m < 0 || r0 > ix->n || m > ix->n - r0) return fail(IVF_EINVAL, "rows outside the index");
  if (m == 0) return IVF_OK;
  ITRY(hipSetDevice(ix->device));
  if (ids) ITRY(hipMemcpy(ids, ix->ids.as<int64_t>() + r0, (size_t)m * 8, hipMemcpyDeviceToHost));
  if (cells) ITRY(hipMemcpy(cells, ix->cell.as<int32_t>() + r0, (size_t)m * 4, hipMemcpyDeviceToHost));
  if (out) ITRY(hipMemcpy(out, (const char *)payload + (size_t)r0 * row_bytes, (size_t)m * row_bytes, hipMemcpyDeviceToHost));
  return IVF_OK;
}

// ---------------------------------------------------------------------------------------------
// the exports both C interfaces have
// ---------------------------------------------------------------------------------------------
int index_info(const IvfBase *ix, int64_t *n, int32_t *d, int32_t *metric, int32_t *nlist) {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (n) *n = ix->n;
  if (d) *d = ix->d;
  if (metric) *metric = ix->metric;
  if (nlist) *nlist = ix->nlist;
  return IVF_OK;
}
int get_centroids(const IvfBase *ix, float *out) {
  if (!ix || !out) return fail(IVF_EINVAL, "null argument");
  DCALL(dann_index_get_vectors(ix->coarse, 0, ix->nlist, out));
  return IVF_OK;
}
int list_sizes(const IvfBase *ix, int64_t *out) {
  if (!ix || !out) return fail(IVF_EINVAL, "null argument");
  std::copy(ix->h_sizes.begin(), ix->h_sizes.end(), out);
  return IVF_OK;
}
int get_assignment(const IvfBase *ix, int64_t *out_ids, int32_t *out_cells) {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (ix->n == 0) return IVF_OK;
  ITRY(hipSetDevice(ix->device));
  if (out_ids) ITRY(hipMemcpy(out_ids, ix->ids.p, (size_t)ix->n * 8, hipMemcpyDeviceToHost));
  if (out_cells) ITRY(hipMemcpy(out_cells, ix->cell.p, (size_t)ix->n * 4, hipMemcpyDeviceToHost));
  return IVF_OK;
}
int last_probes(const IvfBase *ix, int32_t *nq, int32_t *nprobe, int32_t *out_cells) {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (nq) *nq = ix->last_nq;
  if (nprobe) *nprobe = ix->last_nprobe;
  if (out_cells && ix->last_nq > 0) {
    ITRY(hipSetDevice(ix->device));
    ITRY(hipMemcpy(out_cells, ix->probes.p, (size_t)ix->last_nq * ix->last_nprobe * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return IVF_OK;
}
int last_stats(const IvfBase *ix, int64_t *rows_scanned, int32_t *rounds, float *coarse_ms, float *scan_ms, float *select_ms) {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (rows_scanned) *rows_scanned = ix->last_rows;
  if (rounds) *rounds = ix->last_rounds;
  if (coarse_ms) *coarse_ms = ix->t_coarse;
  if (scan_ms) *scan_ms = ix->t_scan;
  if (select_ms) *select_ms = ix->t_sel;
  return IVF_OK;
}

// the index's HNSW quantizer state, with what ivf_hnsw_quantizer.hip needs to know of the index
ivf_hq::State *hq_state(IvfBase *ix) {
  if (!ix) return nullptr;
  ix->hq.device = ix->device;
  ix->hq.metric = ix->metric;
  ix->hq.d = ix->d;
  ix->hq.nlist = ix->nlist;
  ix->hq.coarse = ix->coarse;
  return &ix->hq;
}

}  // namespace
