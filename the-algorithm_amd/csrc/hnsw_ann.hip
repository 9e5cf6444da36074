// hnsw_ann.hip -- HNSW graph search, construction, append and update on gfx950 (include/hnsw_ann.h).  Of the graph the host
// keeps the slot and base tables and one "key exists" flag per row of storage (hnsw_graph_host.h); the lists live on the device,
// and an export reads them from there.  This file is the host side: the index, its helpers, the entry points and the by-id seam.
//   hnsw_queue.h          the one heap (java.util.PriorityQueue) with its entries and orders, Float.compare: host and device
//   hnsw_walk.h           the steps of a walk, each one passage of HnswIndex.java, and the search kernel
//   hnsw_build_kernels.h  the construction, append and update kernels over those steps; the row and key kernels
//   hnsw_host_builder.h   the host-only builder        hnsw_graph_host.h  the host form of the graph
//
// Reference (paths relative to /root/reference/ann/src/main/java/com/twitter/ann/hnsw/):
//   HnswIndex.java:538-553   searchKnn            HnswIndex.java:447-475  bestEntryPointUntilLayer
//   HnswIndex.java:571-623   searchLayerForCandidates
//   HnswIndex.java:137-200,384-440,479-526  insert / mutuallyConnectNewElement / selectNearestNeighboursByHeuristic
//   DistancedItemQueue.java:37-43           queues = java.util.PriorityQueue on Float.compare(distance)
//
// The walk is inherently sequential -- which neighbour is admitted depends on the queue state the
// previous one left -- so the GPU does not parallelise the walk of one query; it runs ~1500 of them
// at once (one wave per query, six waves per CU) and inside a step parallelises what IS parallel:
//   * visited test-and-set for a whole neighbour list: one atomicOr per lane on a per-query bitmap;
//   * distances of the unvisited neighbours: 8 lanes per vector (16-B loads, 128 B contiguous per
//     group), 8 vectors per round, all rounds' loads issued before the first reduction;
//   * then the reference's own admission loop, in list order, on the two queues.
// The queues are java.util.PriorityQueue restated (same siftUp / siftDown), operated wave-uniformly; that makes equal
// distances come out as on the JVM.  What bounds the kernel is how many walks a CU holds -- a walk is one long dependent
// chain of heap steps and gathers, a wave issues an instruction every 3-4 cycles at best (profiles/r03_pmc_c4_dense_hnsw.txt),
// and the LDS a walk needs decides how many waves share a SIMD.  So the LDS holds what is hot and no more: the result queue
// (beam + 1 entries; every admission sifts through it twice) and the TOP of the candidate queue; the candidate queue's tail
// -- which an offer touches at one or two levels and only a poll (one per expansion) descends into -- lives in global
// memory, L2-resident.  ~10 KB per walk = 16 walks per CU at any beam (round 2: 23-39 KB at beam 800, 4-7 walks per CU).
// A query whose candidate queue outgrows the first pass's global part is re-run with a larger one.
// HBM-latency bound by nature: every expansion is a dependent gather of <= 2*maxM random 512-B rows.
//
// Distance arithmetic (the fixed order oracle/hnsw_oracle.c repeats): operands rounded to fp16, fp32
// products and sums, lane j of 8 sums chunks j, j+8, ... of 8 consecutive elements, then a pairwise
// butterfly (xor 1, 2, 4).  Compiled with -ffp-contract=off, so host (builder) == device == oracle.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/hnsw_ann.h"
#include "sann_device.h"  // mix64
#include "ann_by_id_internal.h"
#include "device_buf.h"
#include "host_error.h"
#include "hnsw_graph_host.h"
#include "hnsw_host_builder.h"
#include "hnsw_build_kernels.h"
#define HTRY(expr) HIP_TRY_AS(HNSW_EDEVICE, expr)
#define ABI_CATCH catch (...) { return abi_guard::caught(fail, HNSW_ENOMEM, HNSW_EINTERNAL); }

// ---------------------------------------------------------------------------------------------
// host: the index, the reference's insertion algorithm, the C ABI
// ---------------------------------------------------------------------------------------------
struct hnsw_index {
  int device = 0, metric = 0, d = 0, dpad = 0, m = 0, m0 = 0, max_level = 0;
  int64_t n = 0, entry = -1;
  // The graph (hnsw_graph::FlatGraph): the lists live on the device (`exported` is a read-back), the two small tables on both
  // sides, and the host alone knows which keys HnswNode(level, item) exist besides those with a non-empty list.
  std::vector<int32_t> upper_slot_h, upper_base_h;
  mutable std::vector<uint8_t> has0, has_up;  // [n], [rows of upper_adj]: key loaded or wired, or seen non-empty by an export
  Buf x, adj0, upper_slot, upper_base, upper_adj, ids;
  bool has_ids = false;
  // scratch
  Buf q_in, q, visited, vlog, gc, o_dist, o_ids, o_cnt, spill, stats, qlist;
  bool visited_dirty = true;  // the bitmaps must be wiped before the next search (fresh buffer, or a search that did not finish)
  hipEvent_t ev[2] = {nullptr, nullptr};
  int64_t last_dist = 0, last_exp = 0;
  int32_t last_spilled = 0;
  int64_t last_peak = 0, last_adm = 0;
  float last_ms = 0;
  int64_t build_rounds = 0, build_truncated = 0, build_prunes = 0, build_dropped = 0;  // the last insert_rows (device build, append)
  int64_t search_vwords = 0;  // bitmap layout of the last search: a different one is a fresh layout (visited_dirty)
  // ---- insert_rows (device build, append): room, host-mirror state, and construction scratch kept across calls ----
  int64_t cap = 0;              // rows the per-row buffers (x, adj0, upper_slot, ids, levels) hold; 0 = n
  int64_t upper_rows_cap = 0, upper_slots_cap = 0;
  bool keyed = false;           // created with ids (has_ids may be false only because n was 0)
  bool broken = false;          // a device error part-way through an append: every later call fails with HNSW_EDEVICE
  mutable hnsw_graph::FlatGraph exported;  // the last export's read-back of the device's lists (read_graph) ...
  mutable bool exported_fresh = false;     // ... which no append or update has changed since
  Buf levels;                   // [cap] levels of inserted rows (read by the insert kernel by position)
  Buf b_order, b_pair_off, b_keys, b_sorted, b_tmp, b_bstats, b_visited, b_vlog;
  int64_t bv_items = 0, bv_vwords = 0;  // layout of b_visited: walks at a time, words per walk (reserve_visited)
  bool bv_log = false;          // the walks keep an undo log in b_vlog
  bool bv_clean = false;        // b_visited is all zeros (what a walk with an undo log needs at its start)
  Buf key_table, key_next, key_in, key_batch, key_tmp, key_bad;  // sorted keys of the index (built at the first append)
  int64_t key_n = -1;           // entries of key_table; -1 = not built yet
  // ---- hnsw_index_update ----
  Buf kp_keys, kp_pos, kp_q, kp_out;  // (key, position) sorted by key, built when an update finds n != kp_n
  int64_t kp_n = -1;
  Buf u_pos, u_fmask, u_top, u_pair_off, u_prop_off, u_props, u_pkeys, u_psorted, u_own, u_rows;
  int64_t upd_rounds = 0, upd_relinks = 0, upd_superseded = 0, upd_present = 0, upd_evals = 0, upd_empty = 0;  // the last update
  std::shared_ptr<void> by_id;  // scratch of the by-id queries (ann_by_id.hip), freed with the index
  ~hnsw_index() {
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace {

// the graph of a new handle: its four arrays to the device, its four small ones kept on the host.  A buffer of no rows
// holds one zeroed row, so no kernel is ever handed an allocation shorter than a row.
int upload_graph(hnsw_index *ix, hnsw_graph::FlatGraph &&g) {
  auto put = [](Buf &b, const auto &v, size_t least) {
    hipError_t e = b.reserve(std::max(v.size(), least) * 4);
    if (e == hipSuccess) e = v.empty() ? hipMemset(b.p, 0, least * 4) : hipMemcpy(b.p, v.data(), v.size() * 4, hipMemcpyHostToDevice);
    return e;
  };
  HTRY(put(ix->adj0, g.adj0, (size_t)ix->m0 + 1));
  HTRY(put(ix->upper_slot, g.upper_slot, 1));
  HTRY(put(ix->upper_base, g.upper_base, 1));
  HTRY(put(ix->upper_adj, g.upper_adj, (size_t)ix->m + 1));
  ix->entry = g.entry;
  ix->max_level = g.max_level;
  ix->upper_slot_h = std::move(g.upper_slot);
  ix->upper_base_h = std::move(g.upper_base);
  ix->has0 = std::move(g.has0);
  ix->has_up = std::move(g.has_up);
  return HNSW_OK;
}

// fp32 rows from the host into x from row `at` on, through hnsw_prep_rows, in chunks of 128 MB staged in `stage`
int stage_rows(hnsw_index *ix, Buf &stage, const float *vectors, int64_t n, int64_t at) {
  const int64_t chunk = std::max<int64_t>(1, (int64_t)(128u << 20) / ((int64_t)ix->d * 4));
  HTRY(stage.reserve((size_t)std::min(chunk, n) * ix->d * 4));
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t m = std::min(chunk, n - r0);
    HTRY(hipMemcpy(stage.p, vectors + r0 * ix->d, (size_t)m * ix->d * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(hnsw_prep_rows, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, 0, stage.as<float>(), m, ix->d, ix->dpad,
                       ix->metric == HNSW_METRIC_COSINE ? 1 : 0, ix->x.as<_Float16>() + (at + r0) * ix->dpad);
    HTRY(hipGetLastError());
    if (r0 + chunk < n) HTRY(hipDeviceSynchronize());  // (the next chunk overwrites the staging buffer)
  }
  return HNSW_OK;
}

// the checks every way of making an index shares, and a handle that holds no rows yet
int new_index(int32_t device, int32_t metric, int64_t n, int32_t d, const float *vectors, int32_t max_m, std::unique_ptr<hnsw_index> &ix) {
  if (metric < HNSW_METRIC_L2 || metric > HNSW_METRIC_INNER_PRODUCT) return fail(HNSW_EINVAL, "unknown metric");
  if (n < 0 || n >= (int64_t)0x7fffffff) return fail(HNSW_EINVAL, "vector count out of range");
  if (d < 1 || d > MAX_D) return fail(HNSW_EINVAL, "dimension must be in 1..512");
  if (max_m < 2 || max_m > MAX_M) return fail(HNSW_EINVAL, "max_m must be in 2..32");
  if (n > 0 && !vectors) return fail(HNSW_EINVAL, "NULL vectors");
  ix.reset(new hnsw_index);
  ix->device = device;
  ix->metric = metric;
  ix->d = d;
  ix->dpad = (d + 63) / 64 * 64;
  ix->m = max_m;
  ix->m0 = 2 * max_m;
  HTRY(hipSetDevice(device));
  for (auto &e : ix->ev) HTRY(hipEventCreate(&e));
  return HNSW_OK;
}

// a handle with its rows and ids on the device and no graph yet (upload_graph brings one)
int create_index(int32_t device, int32_t metric, int64_t n, int32_t d, const float *vectors, const int64_t *ids, int32_t max_m,
                 std::unique_ptr<hnsw_index> &ix, std::vector<float> *host_rows) {
  if (int rc = new_index(device, metric, n, d, vectors, max_m, ix)) return rc;
  ix->n = n;
  HTRY(ix->x.reserve((size_t)std::max<int64_t>(n, 1) * ix->dpad * sizeof(_Float16)));
  if (n > 0) {
    Buf stage;
    if (int rc = stage_rows(ix.get(), stage, vectors, n, 0)) return rc;
    HTRY(hipDeviceSynchronize());  // (before the staging buffer is freed)
  }
  if (ids && n > 0) {
    HTRY(ix->ids.reserve((size_t)n * 8));
    HTRY(hipMemcpy(ix->ids.p, ids, (size_t)n * 8, hipMemcpyHostToDevice));
    ix->has_ids = true;
  }
  ix->keyed = ids != nullptr;
  if (host_rows) {  // the stored rows, as floats, for the host-side builder
    std::vector<_Float16> h((size_t)n * ix->dpad);
    if (n > 0) HTRY(hipMemcpy(h.data(), ix->x.p, h.size() * sizeof(_Float16), hipMemcpyDeviceToHost));
    host_rows->resize(h.size());
    for (size_t i = 0; i < h.size(); ++i) (*host_rows)[i] = (float)h[i];
  }
  return HNSW_OK;
}

// levels of the rows at positions first .. first + n - 1: the given ones (each in 0..60), or getRandomLevel
// (HnswIndex.java:369-371) drawn from the seed and the row's position in the whole index
int draw_levels(uint64_t seed, int64_t first, int64_t n, int32_t max_m, const int32_t *given_levels, std::vector<int32_t> &out) {
  out.assign((size_t)std::max<int64_t>(n, 0), 0);
  const double level_mult = 1.0 / std::log(1.0 * max_m);  // HnswIndex.java:118
  for (int64_t i = 0; i < n; ++i) {
    if (given_levels) {
      if (given_levels[i] < 0 || given_levels[i] > 60) return fail(HNSW_EINVAL, "a level is outside 0..60");
      out[(size_t)i] = given_levels[i];
      continue;
    }
    const uint64_t h = sann::mix64(seed ^ ((uint64_t)(first + i) * 0x9E3779B97F4A7C15ull));
    const double u = ((double)(h >> 11) + 1.0) * (1.0 / 9007199254740992.0);  // (0, 1]
    out[(size_t)i] = std::min(60, (int)(-std::log(u) * level_mult));
  }
  return HNSW_OK;
}

// ef_construction and batch of a device build, an append or an update; batch 0 is the default
// (tools/hnsw_update_probe.py: 4096 beats 1024 and 256)
int check_construction_args(int32_t ef_construction, int32_t &batch) {
  if (ef_construction < 1 || ef_construction > BUILD_EF_MAX) return fail(HNSW_EINVAL, "ef_construction must be in 1..256");
  if (batch < 0 || batch > (1 << 20)) return fail(HNSW_EINVAL, "batch must be in 0..2^20");
  if (batch == 0) batch = 4096;
  return HNSW_OK;
}

// rows the per-row buffers must hold for `need` rows: what they hold, or amortised growth (>= 1.5x)
int64_t grown_capacity(const hnsw_index *ix, int64_t need) {
  const int64_t cap = std::max(ix->cap, ix->n);
  return need > cap ? std::max(need, cap + cap / 2) : cap;
}

// the per-row buffers grown to `capacity` rows, device to device; a failed growth leaves the index as it was
int grow_rows(hnsw_index *ix, int64_t capacity) {
  const int64_t n = ix->n;
  HTRY(ix->x.grow_keep((size_t)n * ix->dpad * sizeof(_Float16), (size_t)capacity * ix->dpad * sizeof(_Float16)));
  HTRY(ix->adj0.grow_keep((size_t)n * (ix->m0 + 1) * 4, (size_t)capacity * (ix->m0 + 1) * 4));
  HTRY(ix->upper_slot.grow_keep((size_t)n * 4, (size_t)capacity * 4));
  HTRY(ix->levels.grow_keep(0, (size_t)capacity * 4));
  if (ix->keyed) HTRY(ix->ids.grow_keep((size_t)n * 8, (size_t)capacity * 8));
  ix->cap = capacity;
  return HNSW_OK;
}

// a round's keys (walks write them, back links read them sorted) and the radix sort's scratch, for rounds of up to `max_keys`
int reserve_round_keys(hnsw_index *ix, int64_t max_keys, size_t &tmp_bytes) {
  HTRY(ix->b_keys.reserve((size_t)max_keys * 8));
  HTRY(ix->b_sorted.reserve((size_t)max_keys * 8));
  HTRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, ix->b_keys.as<uint64_t>(), ix->b_sorted.as<uint64_t>(), (int)max_keys, 0, 64, (hipStream_t)0));
  HTRY(ix->b_tmp.reserve(tmp_bytes));
  return HNSW_OK;
}

// The visited bitmaps of construction walks, `max_items` at a time (a round; rounds have at most `batch`), over the capacity
// of the index, and whether the walks keep an undo log (bitmaps of 1 MB and more; tests force it on small graphs by the variable
// read below).  Walks with the log need clean bitmaps and leave them clean, so those are wiped once per layout; walks without it
// wipe their own and leave them dirty.
int reserve_visited(hnsw_index *ix, int64_t max_items, int64_t batch) {
  const int64_t cap = std::max(ix->cap, ix->n), vwords = ((cap + 31) / 32 + 255) / 256 * 256;
  ix->bv_log = vwords >= VLOG_MIN_VWORDS || getenv("HNSW_DEBUG_VLOG") != nullptr;
  if (vwords != ix->bv_vwords || max_items > ix->bv_items) {  // a new layout
    const int64_t items = std::max(max_items, vwords == ix->bv_vwords ? std::min<int64_t>(2 * ix->bv_items, batch) : 0);
    ix->bv_items = ix->bv_vwords = 0;
    ix->bv_clean = false;
    HTRY(ix->b_visited.reserve((size_t)items * vwords * 4));
    ix->bv_items = items;
    ix->bv_vwords = vwords;
  }
  if (ix->bv_log) HTRY(ix->b_vlog.reserve((size_t)ix->bv_items * VLOG_CAP * 4));
  if (ix->bv_log && !ix->bv_clean) HTRY(hipMemsetAsync(ix->b_visited.p, 0, (size_t)ix->bv_items * vwords * 4, 0));
  ix->bv_clean = ix->bv_log;
  return HNSW_OK;
}

// what every construction kernel reads of the index and its scratch (after reserve_visited); the caller adds its work list
BuildArgs build_args(const hnsw_index *ix, int32_t efc) {
  BuildArgs a{};
  a.x = ix->x.as<_Float16>();
  a.adj0 = ix->adj0.as<uint32_t>();
  a.upper_slot = ix->upper_slot.as<int32_t>();
  a.upper_base = ix->upper_base.as<int32_t>();
  a.upper_adj = ix->upper_adj.as<uint32_t>();
  a.visited = ix->b_visited.as<uint32_t>();
  a.vlog = ix->bv_log ? ix->b_vlog.as<uint32_t>() : nullptr;
  a.bstats = ix->b_bstats.as<unsigned long long>();
  a.vwords = ix->bv_vwords;
  a.dpad = ix->dpad;
  a.metric = ix->metric;
  a.m = ix->m;
  a.m0 = ix->m0;
  a.efc = efc;
  a.ccap = BUILD_CCAP;
  if (const char *e = std::getenv("HNSW_BUILD_CCAP")) a.ccap = std::max(2, std::min(BUILD_CCAP, std::atoi(e)));  // (tests: make the prune path run)
  return a;
}

}  // namespace

extern "C" {

const char *hnsw_last_error(void) { return g_err.c_str(); }

int hnsw_index_build(int32_t device, int32_t metric, int64_t n, int32_t d, const float *vectors, const int64_t *ids,
                     int32_t max_m, int64_t entry_point, int32_t max_level, int64_t n_entries, const int32_t *entry_level,
                     const int64_t *entry_item, const int64_t *entry_offsets, const int64_t *entry_neighbours,
                     hnsw_index_t **out) try {
  if (!out) return fail(HNSW_EINVAL, "out is NULL");
  if (n_entries < 0 || (n_entries > 0 && (!entry_level || !entry_item || !entry_offsets)))
    return fail(HNSW_EINVAL, "NULL graph arrays");
  if (entry_point >= n || max_level < 0 || max_level > 64) return fail(HNSW_EINVAL, "entry point / max level out of range");
  std::unique_ptr<hnsw_index> ix;
  int rc = create_index(device, metric, n, d, vectors, ids, max_m, ix, nullptr);
  if (rc) return rc;
  hnsw_graph::FlatGraph g;
  if (const char *bad = hnsw_graph::from_entries(n, max_m, entry_point, max_level, n_entries, entry_level, entry_item, entry_offsets,
                                                 entry_neighbours, g))
    return fail(HNSW_EINVAL, bad);
  rc = upload_graph(ix.get(), std::move(g));
  if (rc) return rc;
  *out = ix.release();
  return HNSW_OK;
} ABI_CATCH

static int build_insert_impl(int32_t device, int32_t metric, int64_t n, int32_t d, const float *vectors, const int64_t *ids,
                             int32_t max_m, int32_t ef_construction, uint64_t seed, const int32_t *given_levels,
                             int32_t n_threads, hnsw_index_t **out);

int hnsw_index_build_insert(int32_t device, int32_t metric, int64_t n, int32_t d, const float *vectors, const int64_t *ids,
                            int32_t max_m, int32_t ef_construction, uint64_t seed, int32_t n_threads, hnsw_index_t **out) try {
  return build_insert_impl(device, metric, n, d, vectors, ids, max_m, ef_construction, seed, nullptr, n_threads, out);
} ABI_CATCH

int hnsw_index_build_insert_levels(int32_t device, int32_t metric, int64_t n, int32_t d, const float *vectors,
                                   const int64_t *ids, int32_t max_m, int32_t ef_construction, const int32_t *levels,
                                   int32_t n_threads, hnsw_index_t **out) try {
  if (!levels && n > 0) return fail(HNSW_EINVAL, "levels is NULL");
  return build_insert_impl(device, metric, n, d, vectors, ids, max_m, ef_construction, 0, levels, n_threads, out);
} ABI_CATCH

static int build_insert_impl(int32_t device, int32_t metric, int64_t n, int32_t d, const float *vectors, const int64_t *ids,
                             int32_t max_m, int32_t ef_construction, uint64_t seed, const int32_t *given_levels,
                             int32_t n_threads, hnsw_index_t **out) {
  if (!out) return fail(HNSW_EINVAL, "out is NULL");
  if (ef_construction < 1) return fail(HNSW_EINVAL, "ef_construction must be positive");
  if (n_threads < 1 || n_threads > 256) return fail(HNSW_EINVAL, "n_threads must be in 1..256");
  std::unique_ptr<hnsw_index> ix;
  std::vector<float> rows;
  int rc = create_index(device, metric, n, d, vectors, ids, max_m, ix, &rows);
  if (rc) return rc;
  std::vector<int32_t> levels;
  rc = draw_levels(seed, 0, n, max_m, given_levels, levels);
  if (rc) return rc;
  HostGraph g;
  g.init(n, max_m, levels);
  HostVectors hv;
  hv.load(rows, n, ix->dpad, metric);
  rows.clear();
  rows.shrink_to_fit();
  insert_all(g, hv, ef_construction, levels, n_threads);
  rc = upload_graph(ix.get(), flat_graph(g));
  if (rc) return rc;
  *out = ix.release();
  return HNSW_OK;
}

static const char *const BROKEN = "an earlier append failed on the device part-way: the index is unusable";

// ---- insertion rounds on the device ------------------------------------------------------------------------------------
// Construction on the device: see the comment above hnsw_build_insert_kernel and include/hnsw_ann.h.  One driver serves the
// one-shot build and the append, because a build is the rounds of an append to an empty graph.  The host works out the
// insertion order of the new rows, the round schedule and the entry point and maxLevel of every round (functions of the
// levels and of the rows already linked alone), grows the buffers device to device, and enqueues kernels; nothing comes back
// before the end, and then only the round counters.  Everything that can be refused is refused before anything changes; from
// the first change on a device error leaves the index broken.  `ids`, for a keyed index, are the new rows' keys.
static int insert_rows(hnsw_index *ix, int64_t n, const float *vectors, const int64_t *ids, const std::vector<int32_t> &lv,
                       int32_t ef_construction, int32_t batch) {
  if (n == 0) return HNSW_OK;
  const int64_t n_old = ix->n;
  // ---- order, rounds, entry point per round (host: functions of the levels and n_old) ----
  std::vector<uint32_t> order((size_t)n);
  for (int64_t i = 0; i < n; ++i) order[(size_t)i] = (uint32_t)i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return lv[x] > lv[y]; });
  struct Round {
    int64_t at, count, entry;
    int max_level;
  };
  std::vector<Round> rounds;
  std::vector<int64_t> pair_off((size_t)n + 1, 0);
  std::vector<int32_t> wired_top((size_t)n, -1);  // layers each new row is wired on (-1: it became the entry of an empty graph)
  int64_t entry = ix->entry, at = 0, linked = n_old, max_keys = 0, max_items = 0;
  int max_level = ix->max_level;
  if (entry < 0) {  // an empty graph: the first row in order is the entry point and is never wired (HnswIndex.java:184-186)
    entry = n_old + order[0];
    max_level = lv[order[0]];
    at = 1;
    linked = n_old + 1;
  }
  while (at < n) {  // the schedule: rounds of min(batch, max(1, linked / 8)) items
    const int64_t m = std::min<int64_t>(n - at, std::min<int64_t>(batch, std::max<int64_t>(1, linked / 8)));
    rounds.push_back({at, m, entry, max_level});
    int64_t up = -1;
    for (int64_t e = at; e < at + m; ++e) {
      const uint32_t r = order[(size_t)e];
      wired_top[r] = std::min(lv[r], max_level);
      pair_off[(size_t)e + 1] = pair_off[(size_t)e] + (int64_t)(wired_top[r] + 1) * ix->m;
      if (up < 0 && lv[r] > max_level) up = r;  // HnswIndex.java:193-198, the round as the unit of interleaving
    }
    max_keys = std::max(max_keys, pair_off[(size_t)(at + m)] - pair_off[(size_t)at]);
    max_items = std::max(max_items, m);
    if (up >= 0) {
      entry = n_old + up;
      max_level = lv[(size_t)up];
    }
    at += m;
    linked += m;
  }
  if (max_keys >= (int64_t)1 << 31) return fail(HNSW_EINVAL, "batch * max_m too large");
  // ---- new upper slots (rows at levels >= 1) at the end ----
  const int64_t old_slots = (int64_t)ix->upper_base_h.size() - 1, old_rows = ix->upper_base_h.back();
  std::vector<int32_t> new_slot((size_t)n, -1), new_base;
  for (int64_t i = 0; i < n; ++i)
    if (lv[(size_t)i] > 0) {
      new_slot[(size_t)i] = (int32_t)(old_slots + (int64_t)new_base.size());
      new_base.push_back((new_base.empty() ? (int32_t)old_rows : new_base.back()) + lv[(size_t)i]);
    }
  const int64_t n_slots = old_slots + (int64_t)new_base.size(), n_rows = new_base.empty() ? old_rows : new_base.back();
  // ---- room: amortised (>= 1.5x), device to device; a failed growth leaves the index as it was ----
  HTRY(hipSetDevice(ix->device));
  if (int rc = grow_rows(ix, grown_capacity(ix, n_old + n))) return rc;
  int64_t slots_cap = std::max(ix->upper_slots_cap, old_slots + 1), rows_cap = std::max(ix->upper_rows_cap, std::max<int64_t>(old_rows, 1));
  if (n_slots + 1 > slots_cap) slots_cap = std::max(n_slots + 1, slots_cap + slots_cap / 2);
  if (n_rows > rows_cap) rows_cap = std::max(n_rows, rows_cap + rows_cap / 2);
  HTRY(ix->upper_base.grow_keep((size_t)(old_slots + 1) * 4, (size_t)slots_cap * 4));
  HTRY(ix->upper_adj.grow_keep((size_t)old_rows * (ix->m + 1) * 4, (size_t)rows_cap * (ix->m + 1) * 4));
  ix->upper_slots_cap = slots_cap;
  ix->upper_rows_cap = rows_cap;
  // construction scratch (kept on the handle)
  size_t tmp_bytes = 0;
  HTRY(ix->b_order.reserve((size_t)n * 4));
  HTRY(ix->b_pair_off.reserve(((size_t)n + 1) * 8));
  HTRY(ix->b_bstats.reserve(4 * 8));
  if (int rc = reserve_round_keys(ix, std::max<int64_t>(max_keys, 1), tmp_bytes)) return rc;
  if (max_items > 0)
    if (int rc = reserve_visited(ix, max_items, batch)) return rc;

  // ---- from here on the index changes: a device error leaves it broken ----
  ix->broken = true;
  if (int rc = stage_rows(ix, ix->q_in, vectors, n, n_old)) return rc;
  if (ix->keyed) HTRY(hipMemcpy(ix->ids.as<int64_t>() + n_old, ids, (size_t)n * 8, hipMemcpyHostToDevice));
  HTRY(hipMemcpy(ix->upper_slot.as<int32_t>() + n_old, new_slot.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  if (!new_base.empty())
    HTRY(hipMemcpy(ix->upper_base.as<int32_t>() + old_slots + 1, new_base.data(), new_base.size() * 4, hipMemcpyHostToDevice));
  HTRY(hipMemsetAsync(ix->adj0.as<uint32_t>() + (size_t)n_old * (ix->m0 + 1), 0, (size_t)n * (ix->m0 + 1) * 4, 0));
  if (n_rows > old_rows)
    HTRY(hipMemsetAsync(ix->upper_adj.as<uint32_t>() + (size_t)old_rows * (ix->m + 1), 0, (size_t)(n_rows - old_rows) * (ix->m + 1) * 4, 0));
  HTRY(hipMemcpy(ix->levels.as<int32_t>() + n_old, lv.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  std::vector<uint32_t> gorder((size_t)n);
  for (int64_t e = 0; e < n; ++e) gorder[(size_t)e] = (uint32_t)(n_old + order[(size_t)e]);
  HTRY(hipMemcpy(ix->b_order.p, gorder.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  HTRY(hipMemcpy(ix->b_pair_off.p, pair_off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
  HTRY(hipMemsetAsync(ix->b_bstats.p, 0, 4 * 8, 0));
  if (max_items > 0) {
    BuildArgs a = build_args(ix, ef_construction);
    a.order = ix->b_order.as<uint32_t>();
    a.levels = ix->levels.as<int32_t>();
    a.pair_off = ix->b_pair_off.as<int64_t>();
    const int chunks = ix->dpad / 64;
    for (const Round &r : rounds) {
      a.entry = (uint32_t)r.entry;  // per round: a row above maxLevel moves the entry point for the rounds after its own
      a.max_level = r.max_level;
      a.at = (uint32_t)r.at;
      a.count = (uint32_t)r.count;
      a.n_keys = (uint32_t)(pair_off[(size_t)(r.at + r.count)] - pair_off[(size_t)r.at]);
      BuildArgs a_ins = a, a_link = a;
      a_ins.keys = ix->b_keys.as<uint64_t>();
      a_link.keys = ix->b_sorted.as<uint64_t>();
      launch_build_any(chunks, a_ins, a_link, 0, 0);
      size_t tb = tmp_bytes;
      HTRY(hipcub::DeviceRadixSort::SortKeys(ix->b_tmp.p, tb, ix->b_keys.as<uint64_t>(), ix->b_sorted.as<uint64_t>(), (int)a.n_keys, 0, 64, (hipStream_t)0));
      launch_build_any(chunks, a_ins, a_link, 0, 1);
      HTRY(hipGetLastError());
    }
  }
  HTRY(hipDeviceSynchronize());
  unsigned long long bs[4] = {0, 0, 0, 0};
  HTRY(hipMemcpy(bs, ix->b_bstats.p, sizeof(bs), hipMemcpyDeviceToHost));
  ix->broken = false;
  // ---- the host side: the new rows' slots and the keys their wiring made (an export reads the lists from the device) ----
  ix->build_truncated = (int64_t)bs[0];
  ix->build_prunes = (int64_t)bs[1];
  ix->build_dropped = (int64_t)bs[2];
  ix->build_rounds = (int64_t)rounds.size();
  ix->n = n_old + n;
  ix->entry = entry;
  ix->max_level = std::max(max_level, 0);
  ix->has_ids = ix->keyed;
  ix->upper_slot_h.resize((size_t)n_old);
  ix->upper_slot_h.insert(ix->upper_slot_h.end(), new_slot.begin(), new_slot.end());
  ix->upper_base_h.insert(ix->upper_base_h.end(), new_base.begin(), new_base.end());
  for (int64_t i = 0; i < n; ++i) {
    ix->has0.push_back(wired_top[(size_t)i] >= 0 ? 1 : 0);
    for (int l = 1; l <= lv[(size_t)i]; ++l) ix->has_up.push_back(l <= wired_top[(size_t)i] ? 1 : 0);
  }
  ix->exported_fresh = false;
  return HNSW_OK;
}

// Construction scratch does not outlive a build: at 50M rows the visited bitmaps of 4096 walks alone are 25.6 GB, beside what
// hnsw_search budgets for itself.  (An append keeps its scratch on purpose; the one after a build makes it anew, `levels`
// too, which is read only for rows being inserted.)
static void release_build_scratch(hnsw_index *ix) {
  for (Buf *b : {&ix->b_order, &ix->b_pair_off, &ix->b_keys, &ix->b_sorted, &ix->b_tmp, &ix->b_bstats, &ix->b_visited, &ix->b_vlog,
                 &ix->levels, &ix->q_in})
    b->release();
  ix->bv_items = ix->bv_vwords = 0;
  ix->bv_clean = false;
}

// the one-shot build: insert_rows over all rows into an empty graph.  Unlike an append it does not look for repeated keys and
// does not build the sorted key table (the first append does).
static int build_insert_gpu_impl(int32_t device, int32_t metric, int64_t n, int32_t d, const float *vectors, const int64_t *ids,
                                 int32_t max_m, int32_t ef_construction, uint64_t seed, const int32_t *given_levels, int32_t batch,
                                 hnsw_index_t **out) {
  if (!out) return fail(HNSW_EINVAL, "out is NULL");
  int rc = check_construction_args(ef_construction, batch);
  if (rc) return rc;
  std::unique_ptr<hnsw_index> ix;
  rc = new_index(device, metric, n, d, vectors, max_m, ix);
  if (rc) return rc;
  std::vector<int32_t> levels;
  rc = draw_levels(seed, 0, n, max_m, given_levels, levels);
  if (rc) return rc;
  rc = upload_graph(ix.get(), hnsw_graph::FlatGraph());  // no rows, no entry point
  if (rc) return rc;
  ix->keyed = ids != nullptr;
  rc = insert_rows(ix.get(), n, vectors, ids, levels, ef_construction, batch);
  if (rc) return rc;
  release_build_scratch(ix.get());
  *out = ix.release();
  return HNSW_OK;
}

int hnsw_index_build_insert_gpu(int32_t device, int32_t metric, int64_t n, int32_t d, const float *vectors, const int64_t *ids,
                                int32_t max_m, int32_t ef_construction, uint64_t seed, int32_t batch, hnsw_index_t **out) try {
  return build_insert_gpu_impl(device, metric, n, d, vectors, ids, max_m, ef_construction, seed, nullptr, batch, out);
} ABI_CATCH

int hnsw_index_build_insert_gpu_levels(int32_t device, int32_t metric, int64_t n, int32_t d, const float *vectors, const int64_t *ids,
                                       int32_t max_m, int32_t ef_construction, const int32_t *levels, int32_t batch, hnsw_index_t **out) try {
  if (!levels && n > 0) return fail(HNSW_EINVAL, "levels is NULL");
  return build_insert_gpu_impl(device, metric, n, d, vectors, ids, max_m, ef_construction, 0, levels, batch, out);
} ABI_CATCH

// ---- hnsw_index_append -------------------------------------------------------------------------------------------------
// insert_rows on a live index, see include/hnsw_ann.h; what is an append's alone is here: the refusals, and for a keyed index the
// first duplicate key, if any (all that comes back besides the round counters), and the sorted table of the keys.
static int append_keys_check(hnsw_index *ix, int64_t n, const int64_t *ids) {
  const int64_t n_old = ix->n;
  size_t tmp_bytes = 0;
  const int64_t most = std::max<int64_t>(std::max<int64_t>(n_old, n), 1);
  HTRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, (const int64_t *)nullptr, (int64_t *)nullptr, (int)most, 0, 64, (hipStream_t)0));
  HTRY(ix->key_tmp.reserve(tmp_bytes));
  if (ix->key_n < 0) {  // the sorted table of the keys already in the index, once
    HTRY(ix->key_table.reserve((size_t)std::max<int64_t>(n_old, 1) * 8));
    if (n_old > 0) {
      size_t tb = tmp_bytes;
      HTRY(hipcub::DeviceRadixSort::SortKeys(ix->key_tmp.p, tb, ix->ids.as<int64_t>(), ix->key_table.as<int64_t>(), (int)n_old, 0, 64, (hipStream_t)0));
    }
    ix->key_n = n_old;
  }
  HTRY(ix->key_in.reserve((size_t)n * 8));
  HTRY(ix->key_batch.reserve((size_t)n * 8));
  HTRY(ix->key_bad.reserve(4));
  HTRY(hipMemcpy(ix->key_in.p, ids, (size_t)n * 8, hipMemcpyHostToDevice));
  size_t tb = tmp_bytes;
  HTRY(hipcub::DeviceRadixSort::SortKeys(ix->key_tmp.p, tb, ix->key_in.as<int64_t>(), ix->key_batch.as<int64_t>(), (int)n, 0, 64, (hipStream_t)0));
  HTRY(hipMemsetAsync(ix->key_bad.p, 0x7f, 4, 0));
  hipLaunchKernelGGL(hnsw_key_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ix->key_table.as<int64_t>(), ix->key_n,
                     ix->key_batch.as<int64_t>(), n, ix->key_bad.as<int32_t>());
  HTRY(hipGetLastError());
  int32_t bad = 0;
  HTRY(hipMemcpy(&bad, ix->key_bad.p, 4, hipMemcpyDeviceToHost));
  if (bad >= 0 && bad < n) {
    int64_t k[2] = {0, 0};
    const int64_t from = bad > 0 ? bad - 1 : bad;
    HTRY(hipMemcpy(k, ix->key_batch.as<int64_t>() + from, (size_t)(bad - from + 1) * 8, hipMemcpyDeviceToHost));
    const int64_t key = k[bad - from];
    if (bad > 0 && k[0] == key) return fail(HNSW_EINVAL, "duplicate key " + std::to_string(key) + ": it appears twice in the appended rows");
    return fail(HNSW_EINVAL, "duplicate key " + std::to_string(key) + ": it is already in the index");
  }
  return HNSW_OK;
}

// the graph as an export emits it, in ix->exported: every list from the device, the tables and the flags from the handle.  Kept
// until an append or an update changes the lists, so that hnsw_index_graph_size and hnsw_index_graph share one read
// (profiles/README.md, host_graph: a second read costs more than the parent's whole first export did)
static int read_graph(const hnsw_index *ix) {
  if (ix->broken) return fail(HNSW_EDEVICE, BROKEN);
  if (ix->exported_fresh) return HNSW_OK;
  hnsw_graph::FlatGraph &g = ix->exported;
  HTRY(hipSetDevice(ix->device));
  g.n = ix->n;
  g.m = ix->m;
  g.m0 = ix->m0;
  g.upper_slot = ix->upper_slot_h;
  g.upper_base = ix->upper_base_h;
  g.adj0.resize((size_t)g.n * (g.m0 + 1));
  g.upper_adj.resize((size_t)g.upper_base.back() * (g.m + 1));
  if (!g.adj0.empty()) HTRY(hipMemcpy(g.adj0.data(), ix->adj0.p, g.adj0.size() * 4, hipMemcpyDeviceToHost));
  if (!g.upper_adj.empty()) HTRY(hipMemcpy(g.upper_adj.data(), ix->upper_adj.p, g.upper_adj.size() * 4, hipMemcpyDeviceToHost));
  // A key, once seen, stays a key, like an entry of the reference's map: a list that an export found non-empty keeps its key
  // on the handle even if an update empties the list later.  This is the one thing an export writes.
  for (int64_t i = 0; i < g.n; ++i) ix->has0[(size_t)i] |= g.adj0[(size_t)i * (g.m0 + 1)] > 0;
  for (size_t r = 0; r < ix->has_up.size(); ++r) ix->has_up[r] |= g.upper_adj[r * (g.m + 1)] > 0;
  g.has0 = ix->has0;
  g.has_up = ix->has_up;
  ix->exported_fresh = true;
  return HNSW_OK;
}

static int append_impl(hnsw_index *ix, int64_t n, const float *vectors, const int64_t *ids, int32_t ef_construction, uint64_t seed,
                       const int32_t *given_levels, int32_t batch) {
  // ---- everything that can be refused is refused before anything changes ----
  if (!ix) return fail(HNSW_EINVAL, "NULL index");
  if (ix->broken) return fail(HNSW_EDEVICE, BROKEN);
  if (n < 0) return fail(HNSW_EINVAL, "n must not be negative");
  if (int rc = check_construction_args(ef_construction, batch)) return rc;
  if (n == 0) return HNSW_OK;
  if (!vectors) return fail(HNSW_EINVAL, "NULL vectors");
  if (ix->keyed && !ids) return fail(HNSW_EINVAL, "the index was created with ids: an append must give ids");
  if (!ix->keyed && ids) return fail(HNSW_EINVAL, "the index was created without ids (its keys are positions): ids must be NULL");
  if (ix->n + n >= (int64_t)0x7fffffff) return fail(HNSW_EINVAL, "the index would reach 2^31 - 1 rows");
  std::vector<int32_t> lv;
  if (int rc = draw_levels(seed, ix->n, n, ix->m, given_levels, lv)) return rc;  // the builder's draw, at the global position
  HTRY(hipSetDevice(ix->device));
  if (ix->keyed) {  // the new keys merged with the sorted table (merge path) into key_next, which is nothing until the tables swap
    if (int rc = append_keys_check(ix, n, ids)) return rc;
    HTRY(ix->key_next.reserve((size_t)grown_capacity(ix, ix->n + n) * 8));
    const int64_t total = ix->key_n + n, threads = (total + MERGE_ITEMS - 1) / MERGE_ITEMS;
    hipLaunchKernelGGL(hnsw_key_merge_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, 0, ix->key_table.as<int64_t>(), ix->key_n,
                       ix->key_batch.as<int64_t>(), n, ix->key_next.as<int64_t>());
    HTRY(hipGetLastError());
  }
  if (int rc = insert_rows(ix, n, vectors, ids, lv, ef_construction, batch)) return rc;  // (it ends with a synchronise: the merge is done)
  if (ix->keyed) {
    std::swap(ix->key_table.p, ix->key_next.p);
    std::swap(ix->key_table.bytes, ix->key_next.bytes);
    ix->key_n += n;
  }
  return HNSW_OK;
}

int hnsw_index_append(hnsw_index_t *ix, int64_t n, const float *vectors, const int64_t *ids, int32_t ef_construction, uint64_t seed,
                      int32_t batch) try {
  return append_impl(ix, n, vectors, ids, ef_construction, seed, nullptr, batch);
} ABI_CATCH

int hnsw_index_append_levels(hnsw_index_t *ix, int64_t n, const float *vectors, const int64_t *ids, int32_t ef_construction,
                             const int32_t *levels, int32_t batch) try {
  if (!levels && n > 0) return fail(HNSW_EINVAL, "levels is NULL");
  return append_impl(ix, n, vectors, ids, ef_construction, 0, levels, batch);
} ABI_CATCH

// ---- hnsw_index_update -------------------------------------------------------------------------------------------------
// Hnsw.update (Hnsw.scala:161-181): keys already in the index are re-inserted (HnswIndex.reInsert, :226-329) in rounds on the
// device, absent ones appended afterwards by append_impl.  See include/hnsw_ann.h for the semantics.

// positions of the requested keys of a keyed index (-1: absent), by the device's (key, position) table
// the device's (key, position) table of a keyed index, sorted by key: (re)built at first use and after an append
static int ensure_key_positions(hnsw_index *ix) {
  const int64_t n_old = ix->n;
  if (ix->kp_n == n_old) return HNSW_OK;
  ix->kp_n = -1;
  size_t tb = 0;
  HTRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const int64_t *)nullptr, (int64_t *)nullptr, (const int64_t *)nullptr,
                                          (int64_t *)nullptr, (int)n_old, 0, 64, (hipStream_t)0));
  Buf tmp, iota;  // (the sort's scratch and the positions it permutes live only for the sort)
  HTRY(tmp.reserve(tb));
  HTRY(iota.reserve((size_t)n_old * 8));
  HTRY(ix->kp_keys.reserve((size_t)n_old * 8));
  HTRY(ix->kp_pos.reserve((size_t)n_old * 8));
  hipLaunchKernelGGL(hnsw_iota_kernel, dim3((unsigned)((n_old + 255) / 256)), dim3(256), 0, 0, iota.as<int64_t>(), n_old);
  HTRY(hipGetLastError());
  HTRY(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, ix->ids.as<int64_t>(), ix->kp_keys.as<int64_t>(), iota.as<int64_t>(),
                                          ix->kp_pos.as<int64_t>(), (int)n_old, 0, 64, (hipStream_t)0));
  HTRY(hipDeviceSynchronize());  // (before tmp and iota are freed)
  ix->kp_n = n_old;
  return HNSW_OK;
}

static int update_positions(hnsw_index *ix, int64_t n, const int64_t *ids, std::vector<int64_t> &pos) {
  const int64_t n_old = ix->n;
  pos.assign((size_t)n, -1);
  if (n_old == 0 || !ix->has_ids) return HNSW_OK;
  if (int rc = ensure_key_positions(ix)) return rc;
  HTRY(ix->kp_q.reserve((size_t)n * 8));
  HTRY(ix->kp_out.reserve((size_t)n * 8));
  HTRY(hipMemcpy(ix->kp_q.p, ids, (size_t)n * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(hnsw_key_lookup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ix->kp_keys.as<int64_t>(),
                     ix->kp_pos.as<int64_t>(), n_old, ix->kp_q.as<int64_t>(), n, ix->kp_out.as<int64_t>());
  HTRY(hipGetLastError());
  HTRY(hipMemcpy(pos.data(), ix->kp_out.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  return HNSW_OK;
}

// the rounds over the present rows: their positions in request order and their rows as given (fp32 [np][d], prepared on the device)
static int update_rounds(hnsw_index *ix, const std::vector<uint32_t> &P, const std::vector<float> &rows, int32_t efc, int32_t batch) {
  const int64_t np = (int64_t)P.size(), B = batch;
  const bool graph_on = ix->entry >= 0;  // (an empty graph: HnswIndex.reInsert's checkState(entryPoint.isPresent); rows alone)
  // ---- host: per item, the layers it has storage for (capped at maxLevel) and the keys the host holds ----
  std::vector<uint64_t> fmask((size_t)np, 0);
  std::vector<int64_t> pair_off((size_t)np + 1, 0), prop_off((size_t)np + 1, 0);
  for (int64_t t = 0; t < np; ++t) {
    const uint32_t p = P[(size_t)t];
    const int32_t sl = ix->upper_slot_h[p];
    const int stor = sl < 0 ? 0 : ix->upper_base_h[(size_t)sl + 1] - ix->upper_base_h[(size_t)sl];
    uint64_t fm = ix->has0[p] ? 1ull : 0ull;
    for (int l = 1; l <= stor && l < 64; ++l)  // (a layer above 63 cannot be named in pkeys either: 6 bits hold the layer)
      if (ix->has_up[(size_t)(ix->upper_base_h[(size_t)sl] + l - 1)]) fm |= 1ull << l;
    fmask[(size_t)t] = fm;
    const int stop = std::min(stor, ix->max_level);
    pair_off[(size_t)t + 1] = pair_off[(size_t)t] + (int64_t)(stop + 1) * ix->m;
    prop_off[(size_t)t + 1] = prop_off[(size_t)t] + (int64_t)(stop + 1) * ix->m0;
  }
  int64_t max_keys = 1, max_props = 1, max_items = 0, n_rounds = 0;
  for (int64_t r0 = 0; r0 < np; r0 += B) {
    const int64_t r1 = std::min(np, r0 + B);
    max_keys = std::max(max_keys, pair_off[(size_t)r1] - pair_off[(size_t)r0]);
    max_props = std::max(max_props, prop_off[(size_t)r1] - prop_off[(size_t)r0]);
    max_items = std::max(max_items, r1 - r0);
    n_rounds++;
  }
  if (max_props >= (int64_t)1 << 27) return fail(HNSW_EINVAL, "batch * max_m too large");
  // ---- scratch (a failed allocation leaves the index as it was) ----
  HTRY(ix->u_pos.reserve((size_t)np * 4));
  HTRY(ix->u_fmask.reserve((size_t)np * 8));
  HTRY(ix->u_top.reserve((size_t)np * 4));
  HTRY(ix->u_pair_off.reserve(((size_t)np + 1) * 8));
  HTRY(ix->u_prop_off.reserve(((size_t)np + 1) * 8));
  HTRY(ix->u_props.reserve((size_t)max_props * (ix->m0 + 1) * 4));
  HTRY(ix->u_pkeys.reserve((size_t)max_props * 8));
  HTRY(ix->u_psorted.reserve((size_t)max_props * 8));
  HTRY(ix->u_own.reserve((size_t)(max_keys / ix->m + 1) * (ix->m + 1) * 4));
  HTRY(ix->u_rows.reserve((size_t)np * ix->d * 4));
  HTRY(ix->b_bstats.reserve(8 * 8));
  size_t tb_keys = 0, tb_props = 0;
  if (int rc = reserve_round_keys(ix, max_keys, tb_keys)) return rc;
  HTRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tb_props, ix->u_pkeys.as<uint64_t>(), ix->u_psorted.as<uint64_t>(), (int)max_props, 0, 64, (hipStream_t)0));
  HTRY(ix->b_tmp.reserve(std::max(tb_keys, tb_props)));
  if (graph_on)
    if (int rc = reserve_visited(ix, max_items, B)) return rc;

  // ---- from here on the index changes: a device error leaves it broken ----
  ix->broken = true;
  HTRY(hipMemcpy(ix->u_rows.p, rows.data(), (size_t)np * ix->d * 4, hipMemcpyHostToDevice));
  HTRY(hipMemcpy(ix->u_pos.p, P.data(), (size_t)np * 4, hipMemcpyHostToDevice));
  HTRY(hipMemcpy(ix->u_fmask.p, fmask.data(), (size_t)np * 8, hipMemcpyHostToDevice));
  HTRY(hipMemcpy(ix->u_pair_off.p, pair_off.data(), ((size_t)np + 1) * 8, hipMemcpyHostToDevice));
  HTRY(hipMemcpy(ix->u_prop_off.p, prop_off.data(), ((size_t)np + 1) * 8, hipMemcpyHostToDevice));
  HTRY(hipMemsetAsync(ix->b_bstats.p, 0, 8 * 8, 0));
  BuildArgs a = build_args(ix, efc);
  a.order = ix->u_pos.as<uint32_t>();
  a.pair_off = ix->u_pair_off.as<int64_t>();
  a.entry = (uint32_t)std::max<int64_t>(ix->entry, 0);  // an update never moves the entry point or maxLevel
  a.max_level = ix->max_level;
  a.utop = ix->u_top.as<int32_t>();
  a.fmask = ix->u_fmask.as<uint64_t>();
  a.prop_off = ix->u_prop_off.as<int64_t>();
  a.props = ix->u_props.as<uint32_t>();
  a.own = ix->u_own.as<uint32_t>();
  const int chunks = ix->dpad / 64;
  for (int64_t r0 = 0; r0 < np; r0 += B) {
    const int64_t r1 = std::min(np, r0 + B), m = r1 - r0;
    a.at = (uint32_t)r0;
    a.count = (uint32_t)m;
    // 1. the round's rows
    hipLaunchKernelGGL(hnsw_update_rows_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, 0, ix->u_rows.as<float>() + r0 * ix->d, m,
                       ix->u_pos.as<uint32_t>() + r0, ix->d, ix->dpad, ix->metric == HNSW_METRIC_COSINE ? 1 : 0, ix->x.as<_Float16>());
    HTRY(hipGetLastError());
    if (!graph_on) continue;
    const int64_t n_pk = prop_off[(size_t)r1] - prop_off[(size_t)r0], n_k = pair_off[(size_t)r1] - pair_off[(size_t)r0];
    // 2. relink: every proposal against the graph as the round found it, then the latest per (layer, v)
    HTRY(hipMemsetAsync(ix->u_pkeys.p, 0xff, (size_t)n_pk * 8, 0));
    BuildArgs ar = a;
    ar.pkeys = ix->u_pkeys.as<uint64_t>();
    launch_update_any(chunks, ar, 0, 0, (unsigned)m);
    size_t tb = tb_props;
    HTRY(hipcub::DeviceRadixSort::SortKeys(ix->b_tmp.p, tb, ix->u_pkeys.as<uint64_t>(), ix->u_psorted.as<uint64_t>(), (int)n_pk, 0, 64, (hipStream_t)0));
    BuildArgs ac = a;
    ac.pkeys = ix->u_psorted.as<uint64_t>();
    ac.n_pkeys = (uint32_t)n_pk;
    hipLaunchKernelGGL(hnsw_update_relink_commit_kernel, dim3((unsigned)((n_pk + 255) / 256)), dim3(256), 0, 0, ac);
    // 3. wire: the walks, then the items' own lists
    HTRY(hipMemsetAsync(ix->b_keys.p, 0xff, (size_t)n_k * 8, 0));
    BuildArgs aw = a;
    aw.keys = ix->b_keys.as<uint64_t>();
    launch_update_any(chunks, aw, 0, 1, (unsigned)m);
    hipLaunchKernelGGL(hnsw_update_own_commit_kernel, dim3((unsigned)m), dim3(64), 0, 0, aw);
    // 4. back links
    tb = tb_keys;
    HTRY(hipcub::DeviceRadixSort::SortKeys(ix->b_tmp.p, tb, ix->b_keys.as<uint64_t>(), ix->b_sorted.as<uint64_t>(), (int)n_k, 0, 64, (hipStream_t)0));
    BuildArgs al = a;
    al.keys = ix->b_sorted.as<uint64_t>();
    al.n_keys = (uint32_t)n_k;
    launch_update_any(chunks, al, 0, 2, (unsigned)n_k);
    HTRY(hipGetLastError());
  }
  HTRY(hipDeviceSynchronize());
  unsigned long long bs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HTRY(hipMemcpy(bs, ix->b_bstats.p, sizeof(bs), hipMemcpyDeviceToHost));
  ix->broken = false;
  ix->exported_fresh = false;
  ix->upd_rounds = n_rounds;
  ix->upd_empty = (int64_t)bs[3];
  ix->upd_relinks = (int64_t)bs[4];
  ix->upd_superseded = (int64_t)bs[5];
  ix->upd_present = (int64_t)bs[6];
  ix->upd_evals = (int64_t)bs[7];
  return HNSW_OK;
}

static int update_impl(hnsw_index *ix, int64_t n, const float *vectors, const int64_t *ids, int32_t ef_construction, uint64_t seed,
                       int32_t batch, int64_t *out_appended) {
  if (out_appended) *out_appended = 0;
  // ---- everything that can be refused is refused before anything changes ----
  if (!ix) return fail(HNSW_EINVAL, "NULL index");
  if (ix->broken) return fail(HNSW_EDEVICE, BROKEN);
  if (n < 0) return fail(HNSW_EINVAL, "n must not be negative");
  if (int rc = check_construction_args(ef_construction, batch)) return rc;
  if (n == 0) return HNSW_OK;
  if (!vectors || !ids) return fail(HNSW_EINVAL, "NULL vectors or ids");
  {
    std::vector<int64_t> sorted(ids, ids + n);
    std::sort(sorted.begin(), sorted.end());
    for (int64_t i = 1; i < n; ++i)
      if (sorted[(size_t)i] == sorted[(size_t)i - 1])
        return fail(HNSW_EINVAL, "key " + std::to_string(sorted[(size_t)i]) + " appears twice in the update");
  }
  const int64_t n_old = ix->n;
  HTRY(hipSetDevice(ix->device));
  std::vector<int64_t> pos;
  if (ix->keyed) {
    const int rc = update_positions(ix, n, ids, pos);
    if (rc) return rc;
  } else {
    for (int64_t i = 0; i < n; ++i)
      if (ids[i] < 0 || ids[i] >= n_old)
        return fail(HNSW_EINVAL, "position " + std::to_string(ids[i]) + " is not in the index (its keys are positions 0.." +
                                     std::to_string(n_old - 1) + ")");
    pos.assign(ids, ids + n);
  }
  std::vector<uint32_t> P;
  std::vector<float> rows, arows;
  std::vector<int64_t> akeys;
  for (int64_t i = 0; i < n; ++i) {
    const float *v = vectors + (size_t)i * ix->d;
    if (pos[(size_t)i] >= 0) {
      P.push_back((uint32_t)pos[(size_t)i]);
      rows.insert(rows.end(), v, v + ix->d);
    } else {
      akeys.push_back(ids[i]);
      arows.insert(arows.end(), v, v + ix->d);
    }
  }
  if (n_old + (int64_t)akeys.size() >= (int64_t)0x7fffffff) return fail(HNSW_EINVAL, "the index would reach 2^31 - 1 rows");
  ix->upd_rounds = ix->upd_relinks = ix->upd_superseded = ix->upd_present = ix->upd_evals = ix->upd_empty = 0;
  if (!P.empty()) {
    const int rc = update_rounds(ix, P, rows, ef_construction, batch);
    if (rc) return rc;
  }
  if (!akeys.empty()) {  // Hnsw.update of a new key: insert (Hnsw.scala:172-173), by the append path, in request order
    const int rc = append_impl(ix, (int64_t)akeys.size(), arows.data(), akeys.data(), ef_construction, seed, nullptr, batch);
    if (rc && !P.empty())  // (everything refusable was refused above: this is the append running out of room, or the device)
      return fail(rc, std::string("the present keys were updated, the absent ones not appended: ") + hnsw_last_error());
    if (rc) return rc;
    if (out_appended) *out_appended = (int64_t)akeys.size();
  }
  return HNSW_OK;
}

int hnsw_index_update(hnsw_index_t *ix, int64_t n, const float *vectors, const int64_t *ids, int32_t ef_construction, uint64_t seed,
                      int32_t batch, int64_t *out_appended) try {
  return update_impl(ix, n, vectors, ids, ef_construction, seed, batch, out_appended);
} ABI_CATCH

int hnsw_index_update_stats(const hnsw_index_t *ix, int64_t *rounds, int64_t *relinks, int64_t *relinks_superseded,
                            int64_t *additions_already_present, int64_t *distance_evals, int64_t *lists_kept) try {
  if (!ix) return fail(HNSW_EINVAL, "NULL index");
  if (rounds) *rounds = ix->upd_rounds;
  if (relinks) *relinks = ix->upd_relinks;
  if (relinks_superseded) *relinks_superseded = ix->upd_superseded;
  if (additions_already_present) *additions_already_present = ix->upd_present;
  if (distance_evals) *distance_evals = ix->upd_evals;
  if (lists_kept) *lists_kept = ix->upd_empty;
  return HNSW_OK;
} ABI_CATCH

int hnsw_index_reserve(hnsw_index_t *ix, int64_t capacity) try {
  if (!ix) return fail(HNSW_EINVAL, "NULL index");
  if (ix->broken) return fail(HNSW_EDEVICE, BROKEN);
  if (capacity < 0 || capacity >= (int64_t)0x7fffffff) return fail(HNSW_EINVAL, "capacity out of range");
  const int64_t n = ix->n;
  if (capacity <= std::max(ix->cap, n)) return HNSW_OK;  // never shrinks
  HTRY(hipSetDevice(ix->device));
  if (int rc = grow_rows(ix, capacity)) return rc;
  if (ix->keyed) {
    if (ix->key_n >= 0) HTRY(ix->key_table.grow_keep((size_t)ix->key_n * 8, (size_t)capacity * 8));
    HTRY(ix->key_next.reserve((size_t)capacity * 8));
  }
  return HNSW_OK;
} ABI_CATCH

int hnsw_index_build_stats(const hnsw_index_t *ix, int64_t *rounds, int64_t *unseen_additions, int64_t *queue_prunes, int64_t *dropped_candidates) try {
  if (!ix) return fail(HNSW_EINVAL, "NULL index");
  if (rounds) *rounds = ix->build_rounds;
  if (unseen_additions) *unseen_additions = ix->build_truncated;
  if (queue_prunes) *queue_prunes = ix->build_prunes;
  if (dropped_candidates) *dropped_candidates = ix->build_dropped;
  return HNSW_OK;
} ABI_CATCH

int hnsw_index_graph_size(const hnsw_index_t *ix, int64_t *n_entries, int64_t *n_neighbours, int64_t *entry_point,
                          int32_t *max_level) try {
  if (!ix) return fail(HNSW_EINVAL, "NULL index");
  if (int rc = read_graph(ix)) return rc;
  int64_t ne = 0, nn = 0;
  hnsw_graph::count_entries(ix->exported, &ne, &nn);
  if (n_entries) *n_entries = ne;
  if (n_neighbours) *n_neighbours = nn;
  if (entry_point) *entry_point = ix->entry;
  if (max_level) *max_level = ix->max_level;
  return HNSW_OK;
} ABI_CATCH

int hnsw_index_graph(const hnsw_index_t *ix, int32_t *entry_level, int64_t *entry_item, int64_t *entry_offsets,
                     int64_t *entry_neighbours) try {
  if (!ix || !entry_level || !entry_item || !entry_offsets) return fail(HNSW_EINVAL, "NULL argument");
  if (int rc = read_graph(ix)) return rc;
  hnsw_graph::emit_entries(ix->exported, entry_level, entry_item, entry_offsets, entry_neighbours);
  return HNSW_OK;
} ABI_CATCH

int hnsw_index_get_vectors(const hnsw_index_t *ix, int64_t i0, int64_t n, float *out) try {
  if (!ix || !out || i0 < 0 || n < 0 || i0 + n > ix->n) return fail(HNSW_EINVAL, "range outside the index");
  if (ix->broken) return fail(HNSW_EDEVICE, BROKEN);
  if (n == 0) return HNSW_OK;
  HTRY(hipSetDevice(ix->device));
  // in slabs: a launch stays far below 2^32 work-items (50M x 256 elements in ONE launch is 1.28e10 -- the grid wrapped and
  // most of the buffer came back unwritten: profiles/r03_hnsw_bench_50M_*) and the staging buffer below 1 GiB
  const int64_t slab = std::max<int64_t>(1, ((int64_t)1 << 28) / ix->d);  // rows per launch: <= 2^28 elements
  Buf tmp;
  HTRY(tmp.reserve((size_t)std::min(slab, n) * ix->d * 4));
  for (int64_t r0 = 0; r0 < n; r0 += slab) {
    const int64_t m = std::min(slab, n - r0), e = m * ix->d;
    hipLaunchKernelGGL(hnsw_rows_to_f32, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, 0, ix->x.as<_Float16>(), i0 + r0, m, ix->d,
                       ix->dpad, tmp.as<float>());
    HTRY(hipGetLastError());
    HTRY(hipMemcpy(out + (size_t)r0 * ix->d, tmp.p, (size_t)e * 4, hipMemcpyDeviceToHost));
  }
  return HNSW_OK;
} ABI_CATCH

int hnsw_index_info(const hnsw_index_t *ix, int64_t *n, int32_t *d, int32_t *metric, int32_t *max_m) try {
  if (!ix) return fail(HNSW_EINVAL, "NULL index");
  if (n) *n = ix->n;
  if (d) *d = ix->d;
  if (metric) *metric = ix->metric;
  if (max_m) *max_m = ix->m;
  return HNSW_OK;
} ABI_CATCH

int hnsw_index_get_ids(const hnsw_index_t *ix, int64_t *out) try {
  if (!ix || (!out && ix->n > 0)) return fail(HNSW_EINVAL, "NULL argument");
  if (ix->broken) return fail(HNSW_EDEVICE, BROKEN);
  if (ix->n == 0) return HNSW_OK;
  if (!ix->has_ids) {
    for (int64_t i = 0; i < ix->n; ++i) out[i] = i;
    return HNSW_OK;
  }
  HTRY(hipSetDevice(ix->device));
  HTRY(hipMemcpy(out, ix->ids.p, (size_t)ix->n * 8, hipMemcpyDeviceToHost));
  return HNSW_OK;
} ABI_CATCH

int hnsw_index_destroy(hnsw_index_t *ix) try {
  delete ix;
  return HNSW_OK;
} ABI_CATCH

// The second half of a search: the walks over the first nq rows of the prepared-query buffer ix->q (fp16 [nq][dpad]), the second
// pass for the queries that outgrow their queues included.  Ends synchronised with the answers in o_dist / o_ids / o_cnt on
// the device.  hnsw_search and the by-id query (ann_by_id.hip) share it.  h2d / d2h: the control bytes it moved.
static int search_prepared(hnsw_index *ix, int32_t nq, int32_t k, int beam, int64_t *h2d, int64_t *d2h) {
  *h2d = *d2h = 0;
  HTRY(hipSetDevice(ix->device));
  const int64_t vwords = (ix->n + 31) / 32;
  // concurrent queries per launch: bounded by the visited bitmaps -- n bits per query, up to 48 GiB of the 288 (at 50M
  // vectors a bitmap is 6.25 MB; the 2 GiB this was capped at until round 3 let 343 walks run at a time, 1.3 per CU,
  // and a 4096-query batch took twelve launches: profiles/r03_hnsw_bench_50M_*)
  int64_t per_launch = std::min<int64_t>(nq, std::max<int64_t>(64, (int64_t)(48ull << 30) / (vwords * 4)));
  per_launch = std::min<int64_t>(per_launch, 1 << 16);
  {
    const void *before = ix->visited.p;
    HTRY(ix->visited.reserve((size_t)per_launch * vwords * 4));
    if (ix->visited.p != before || vwords != ix->search_vwords) ix->visited_dirty = true;  // a new buffer or a new layout (appends grow n)
    ix->search_vwords = vwords;
  }
  const bool use_vlog = vwords >= VLOG_MIN_VWORDS || getenv("HNSW_DEBUG_VLOG") != nullptr;  // (the variable: tests force the log on small graphs)
  HTRY(ix->o_dist.reserve((size_t)nq * k * 4));
  HTRY(ix->o_ids.reserve((size_t)nq * k * 8));
  HTRY(ix->o_cnt.reserve((size_t)nq * 4));
  HTRY(ix->spill.reserve((size_t)nq * 4));
  HTRY(ix->stats.reserve(128));
  hipStream_t st = 0;
  HTRY(hipMemsetAsync(ix->stats.p, 0, 128, st));
  HTRY(hipMemsetAsync(ix->spill.p, 0, (size_t)nq * 4, st));

  SearchArgs a;
  a.x = ix->x.as<_Float16>();
  a.adj0 = ix->adj0.as<uint32_t>();
  a.upper_slot = ix->upper_slot.as<int32_t>();
  a.upper_base = ix->upper_base.as<int32_t>();
  a.upper_adj = ix->upper_adj.as<uint32_t>();
  a.ids = ix->has_ids ? ix->ids.as<int64_t>() : nullptr;
  a.visited = ix->visited.as<uint32_t>();
  if (use_vlog) HTRY(ix->vlog.reserve((size_t)per_launch * VLOG_CAP * 4));
  a.vlog = use_vlog ? ix->vlog.as<uint32_t>() : nullptr;
  a.gc = nullptr;
  a.out_dist = ix->o_dist.as<float>();
  a.out_ids = ix->o_ids.as<int64_t>();
  a.out_counts = ix->o_cnt.as<int32_t>();
  a.spill = ix->spill.as<int32_t>();
  a.stats = ix->stats.as<unsigned long long>();
  a.vwords = vwords;
  a.dpad = ix->dpad;
  a.chunks = ix->dpad / 64;
  a.m = ix->m;
  a.m0 = ix->m0;
  a.metric = ix->metric;
  a.k = k;
  a.ef = beam;
  a.max_level = ix->max_level;
  a.entry = (uint32_t)ix->entry;
  // Every admission enters the candidate queue and stale ones stay: it reaches 2-3x the beam on clustered data and far more
  // on structureless data (i.i.d. Gaussians).  Its top is in LDS -- as much as WALK_LDS_BYTES leaves beside the result queue
  // -- and the rest in global memory: CCAP_FIRST entries per query in the first pass, CCAP_GLOBAL for the queries that
  // outgrow that (pass 2, at most 256 at a time).
  int lds_n = std::max(64, std::min(CCAP_LDS, (int)((WALK_LDS_BYTES - (size_t)(beam + 1) * sizeof(KEntry)) / sizeof(KEntry))));
  if (search_lds_bytes(beam, 64) > (size_t)WALK_LDS_BYTES) lds_n = 64;
  int gcap_first = CCAP_FIRST;
  if (const char *e = getenv("HNSW_DEBUG_CCAP")) {  // tests: v > 0: v entries in LDS and v in the first pass's global part (so queries spill into pass 2); v < 0: |v| in LDS, the usual global part
    const int v = atoi(e);
    lds_n = std::min(CCAP_LDS, std::max(1, v < 0 ? -v : v));
    if (v > 0) gcap_first = v;
  }

  // the visited bitmaps: wiped when the buffer is new (or a search was cut short); every walk leaves its own clean (visited_undo)
  if (use_vlog && ix->visited_dirty) HTRY(hipMemsetAsync(ix->visited.p, 0, ix->visited.bytes, st));
  ix->visited_dirty = true;  // (until this search has run to its end)
  HTRY(hipEventRecord(ix->ev[0], st));
  std::vector<int32_t> redo, spill((size_t)nq);
  for (int pass = 0; pass < 2; ++pass) {
    const bool first = pass == 0;
    if (!first && redo.empty()) break;
    const int64_t todo = first ? nq : (int64_t)redo.size();
    const int gcap = first ? gcap_first : CCAP_GLOBAL;
    int64_t batch = std::min<int64_t>(per_launch, first ? (int64_t)1 << 16 : 256);
    batch = std::min<int64_t>(batch, todo);
    HTRY(ix->gc.reserve((size_t)batch * gcap * sizeof(KEntry)));
    if (!first) {
      HTRY(ix->qlist.reserve(redo.size() * 4));
      HTRY(hipMemcpyAsync(ix->qlist.p, redo.data(), redo.size() * 4, hipMemcpyHostToDevice, st));
      *h2d += (int64_t)redo.size() * 4;
    }
    for (int64_t r0 = 0; r0 < todo; r0 += batch) {
      const int64_t m = std::min<int64_t>(batch, todo - r0);
      if (!use_vlog) HTRY(hipMemsetAsync(ix->visited.p, 0, (size_t)m * vwords * 4, st));
      SearchArgs b = a;
      if (first) {
        b.q = ix->q.as<_Float16>() + r0 * ix->dpad;
        b.qlist = nullptr;
        b.out_dist = a.out_dist + r0 * k;
        b.out_ids = a.out_ids + r0 * k;
        b.out_counts = a.out_counts + r0;
        b.spill = a.spill + r0;
      } else {
        b.q = ix->q.as<_Float16>();
        b.qlist = ix->qlist.as<int32_t>() + r0;
      }
      b.gc = ix->gc.as<KEntry>();
      b.ccap_lds = lds_n;
      b.gcap = gcap;
      int rc = launch_search_any(a.chunks, (int)m, b, st);
      if (rc) return rc;
      HTRY(hipGetLastError());
    }
    HTRY(hipMemcpyAsync(spill.data(), ix->spill.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    *d2h += (int64_t)nq * 4;
    HTRY(hipStreamSynchronize(st));
    std::vector<int32_t> still;
    if (first) {
      for (int32_t q = 0; q < nq; ++q)
        if (spill[(size_t)q]) still.push_back(q);
      ix->last_spilled = (int32_t)still.size();
    } else {
      for (int32_t q : redo)
        if (spill[(size_t)q]) still.push_back(q);
    }
    redo.swap(still);
  }
  if (!redo.empty()) return fail(HNSW_ELIMIT, "candidate queue above 131072 entries");
  HTRY(hipEventRecord(ix->ev[1], st));
  unsigned long long stats[16] = {0};
  HTRY(hipMemcpyAsync(stats, ix->stats.p, 128, hipMemcpyDeviceToHost, st));
  *d2h += 128;
  HTRY(hipStreamSynchronize(st));
  ix->visited_dirty = !use_vlog;
  ix->last_dist = (int64_t)stats[0];
  ix->last_exp = (int64_t)stats[1];
  ix->last_peak = (int64_t)stats[2];
  ix->last_adm = (int64_t)stats[3];
  (void)hipEventElapsedTime(&ix->last_ms, ix->ev[0], ix->ev[1]);
  return HNSW_OK;
}

int hnsw_search(hnsw_index_t *ix, int32_t nq, const float *queries, int32_t k, int32_t ef, float *out_dist, int64_t *out_ids,
                int32_t *out_counts) try {
  if (!ix || !queries || !out_dist || !out_ids || !out_counts) return fail(HNSW_EINVAL, "NULL argument");
  if (nq < 1) return fail(HNSW_EINVAL, "nq must be positive");
  if (k < 1 || ef < 1) return fail(HNSW_EINVAL, "k and ef must be positive");
  const int beam = std::max(ef, k);  // HnswIndex.java:545
  if (beam > MAX_EF) return fail(HNSW_ELIMIT, "max(ef, k) above 1024");
  if (ix->broken) return fail(HNSW_EDEVICE, BROKEN);
  ix->last_dist = ix->last_exp = 0;
  ix->last_spilled = 0;
  ix->last_ms = 0;
  if (ix->entry < 0) {  // metadata.getEntryPoint() absent: Collections.emptyList() (:550-552)
    for (int32_t q = 0; q < nq; ++q) out_counts[q] = 0;
    return HNSW_OK;
  }
  HTRY(hipSetDevice(ix->device));
  HTRY(ix->q_in.reserve((size_t)nq * ix->d * 4));
  HTRY(ix->q.reserve((size_t)nq * ix->dpad * sizeof(_Float16)));
  hipStream_t st = 0;
  HTRY(hipMemcpyAsync(ix->q_in.p, queries, (size_t)nq * ix->d * 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(hnsw_prep_rows, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, ix->q_in.as<float>(), (int64_t)nq, ix->d,
                     ix->dpad, ix->metric == HNSW_METRIC_COSINE ? 1 : 0, ix->q.as<_Float16>());
  HTRY(hipGetLastError());
  int64_t h2d = 0, d2h = 0;
  if (int rc = search_prepared(ix, nq, k, beam, &h2d, &d2h)) return rc;
  HTRY(hipMemcpyAsync(out_dist, ix->o_dist.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, st));
  HTRY(hipMemcpyAsync(out_ids, ix->o_ids.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost, st));
  HTRY(hipMemcpyAsync(out_counts, ix->o_cnt.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
  HTRY(hipStreamSynchronize(st));
  return HNSW_OK;
} ABI_CATCH

int hnsw_last_stats(const hnsw_index_t *ix, int64_t *distance_evals, int64_t *expansions, int32_t *spilled_queries,
                    float *kernel_ms) try {
  if (!ix) return fail(HNSW_EINVAL, "NULL index");
  if (distance_evals) *distance_evals = ix->last_dist;
  if (expansions) *expansions = ix->last_exp;
  if (spilled_queries) *spilled_queries = ix->last_spilled;
  if (kernel_ms) *kernel_ms = ix->last_ms;
  return HNSW_OK;
} ABI_CATCH

int hnsw_last_walk_counters(const hnsw_index_t *ix, int64_t *admissions, int64_t *largest_candidate_queue) try {
  if (!ix) return fail(HNSW_EINVAL, "NULL index");
  if (admissions) *admissions = ix->last_adm;
  if (largest_candidate_queue) *largest_candidate_queue = ix->last_peak;
  return HNSW_OK;
} ABI_CATCH

}  // extern "C"


// ---- the seam of the by-id queries (ann_by_id_internal.h) ----
namespace ann_by_id {

int hnsw_open(hnsw_index *ix, int32_t nq_cap, int32_t k, int32_t ef, bool own_keys, HnswTarget *out) {
  if (!ix || !out) return fail(HNSW_EINVAL, "NULL argument");
  if (k < 1 || ef < 1) return fail(HNSW_EINVAL, "k and ef must be positive");
  if (std::max(ef, k) > MAX_EF) return fail(HNSW_ELIMIT, "max(ef, k) above 1024");
  if (ix->broken) return fail(HNSW_EDEVICE, BROKEN);
  HTRY(hipSetDevice(ix->device));
  HTRY(ix->q.reserve((size_t)std::max(nq_cap, 1) * ix->dpad * sizeof(_Float16)));
  if (own_keys && ix->has_ids && ix->n > 0)
    if (int rc = ensure_key_positions(ix)) return rc;
  out->device = ix->device;
  out->metric = ix->metric;
  out->d = ix->d;
  out->dpad = ix->dpad;
  out->n = ix->n;
  out->empty = ix->entry < 0;
  out->q = ix->q.as<_Float16>();
  out->x = ix->x.as<_Float16>();
  const bool table = own_keys && ix->has_ids && ix->n > 0;
  out->kp_keys = table ? ix->kp_keys.as<int64_t>() : nullptr;
  out->kp_pos = table ? ix->kp_pos.as<int64_t>() : nullptr;
  out->kp_n = table ? ix->kp_n : 0;
  return HNSW_OK;
}

int hnsw_search_prepared(hnsw_index *ix, int32_t nq, int32_t k, int32_t ef, DeviceResult *out) {
  ix->last_dist = ix->last_exp = 0;
  ix->last_spilled = 0;
  ix->last_ms = 0;
  if (int rc = search_prepared(ix, nq, k, std::max(ef, k), &out->h2d_bytes, &out->d2h_bytes)) return rc;
  out->dist = ix->o_dist.as<float>();
  out->ids = ix->o_ids.as<int64_t>();
  out->counts = ix->o_cnt.as<int32_t>();
  return HNSW_OK;
}

std::shared_ptr<void> &hnsw_scratch(hnsw_index *ix) { return ix->by_id; }

}  // namespace ann_by_id
