// annoy_ann.hip -- the Annoy index on the device (include/annoy_ann.h) for gfx950: a forest built and validated on the host
// (annoy_forest.cpp), the best-first walk, the exact re-score of the collected rows and the selection.
//
// What it replaces: RawAnnoyQueryIndex.scala:124-138 hands nodesToExplore to the library's get_nns_by_vector; the contract
// -- the queue's order, the margin's arithmetic, the stop rule -- is the header's.
//
// Shape of the computation, per slice of queries (a slice is what the scratch budget admits):
//   * walk_kernel: one wave per query.  The prepared query sits in registers (a lane holds its one or two pieces of 8
//     components as fp32); the 64 lanes share each margin (one 16-byte load per lane and piece, the xor tree).  The
//     priority queue is a binary max-heap of 64-bit keys (f2key(bound) << 32 | node: the header's order is the integer
//     order) in per-query global scratch, which L2 holds; lane 0 alone reads and writes it and broadcasts what it popped.
//     A leaf's items go, 64 at a time, through a per-query open-addressing set (atomicCAS on a table twice the largest
//     candidate count); the new ones are appended to the query's candidate list at slots a ballot assigns, so the list
//     does not depend on which lane won which table slot.  Every loop is bounded: pops by the node count, probes by the
//     table size.  A query whose heap would outgrow the first launch's capacity is flagged and walked again with room for
//     every node (a node enters the queue at most once), so no answer depends on the capacity.
//   * score_kernel: row_score.h's distance, the one refine_ann.hip re-ranks by (one wave per candidate row, four rows in
//     flight); the distance goes with the row's rank in (id, position) order into a 64-bit key, unique per candidate.
//   * select_kernel: one workgroup per query.  Up to 1024 candidates are sorted in LDS (sort_keys_desc of survivor_topk.h
//     over the complemented keys); more than that first find the k-th smallest key by 8 radix passes over an LDS histogram
//     and gather the k keys at or below it.  row_score.h's emit writes the answer.  No floating-point atomics anywhere.
// No kernel waits on another workgroup.  A forest reaches the device only through annoy_forest_load's validation or the
// builder.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/annoy_ann.h"
#include "abi_guard.h"
#include "annoy_forest.h"
#include "device_buf.h"
#include "row_score.h"  // load_query, load_pieces, wave_sum_f32, score_rows, emit_sorted; survivor_topk.h's f2key, key2f, sort_keys_desc

namespace {

using annoy_host::fail;
#define ATRY(expr)                                                                                       \
  do {                                                                                                   \
    hipError_t e_ = (expr);                                                                              \
    if (e_ != hipSuccess) return fail(IVF_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));   \
  } while (0)
#define ABI_CATCH catch (...) { return abi_guard::caught(fail, IVF_ENOMEM, IVF_EINTERNAL); }

constexpr uint32_t EMPTY = 0xffffffffu;
constexpr int SELECT_LDS = 1024;                       // keys sorted in LDS: ANNOY_MAX_K
constexpr int64_t DEFAULT_QUEUE = 16384;               // first launch: room for the roots and this many more entries
constexpr int64_t DEFAULT_BUDGET = 512ll << 20;        // scratch of one launch
constexpr int64_t KEEP_CANDIDATES = 256ll << 20;       // candidate lists of a whole batch are kept up to this size

struct WalkArgs {
  const int4 *nodes;          // (kind | flags << 1, a, b, split number)
  const _Float16 *normals;    // [n_splits][stride]
  const float *offsets;
  const int32_t *roots;
  const int32_t *items;
  const _Float16 *q16;        // prepared queries of the slice, [m][stride]
  const int32_t *qlist;       // the queries of this launch (slice-local), or null: 0..m-1
  unsigned long long *heap;   // [launch-local query][heap_cap]
  uint32_t *table;            // [slice-local query][table_cap], EMPTY before the launch
  int32_t *cand;              // [slice-local query][cand_cap]
  int32_t *cnt, *pops, *collected, *flags;  // [slice-local query]
  uint32_t n_nodes, heap_cap, table_cap, cand_cap, search_k;
  int32_t m, n_trees, stride, l2;
};

__device__ __forceinline__ unsigned long long queue_key(float bound, uint32_t node) {
  if (bound == 0.0f) bound = 0.0f;  // -0 counts as +0
  return ((unsigned long long)f2key(bound) << 32) | node;
}

// lane 0's heap: a binary max-heap of `size` keys
__device__ __forceinline__ void heap_push(unsigned long long *h, uint32_t &size, unsigned long long key) {
  uint32_t i = size++;
  while (i > 0) {
    const uint32_t p = (i - 1) >> 1;
    const unsigned long long pk = h[p];
    if (pk >= key) break;
    h[i] = pk;
    i = p;
  }
  h[i] = key;
}
__device__ __forceinline__ unsigned long long heap_pop(unsigned long long *h, uint32_t &size) {
  const unsigned long long top = h[0];
  const unsigned long long last = h[--size];
  uint32_t i = 0;
  for (;;) {
    uint32_t c = 2 * i + 1;
    if (c >= size) break;
    unsigned long long ck = h[c];
    if (c + 1 < size) {
      const unsigned long long rk = h[c + 1];
      if (rk > ck) {
        ck = rk;
        ++c;
      }
    }
    if (ck <= last) break;
    h[i] = ck;
    i = c;
  }
  if (size > 0) h[i] = last;
  return top;
}

// One wave per query, four waves per workgroup, NP as row_score.h has it.  The margin's arithmetic is the header's (the
// pieces and the lane sums' tree are row_score.h's; the multiply-add is here); the file is compiled with -ffp-contract=off.
template <int NP>
__global__ __launch_bounds__(256) void walk_kernel(WalkArgs a) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= a.m) return;  // (the same for every lane of a wave)
  const int q = a.qlist ? a.qlist[w] : w;
  const int pieces = a.stride >> 3;
  float qf[NP][8];
  load_query<NP>(a.q16 + (size_t)q * a.stride, pieces, qf);
  unsigned long long *heap = a.heap + (size_t)w * a.heap_cap;
  uint32_t *table = a.table + (size_t)q * a.table_cap;
  int32_t *cand = a.cand + (size_t)q * a.cand_cap;
  const uint32_t mask = a.table_cap - 1;

  uint32_t size = 0;  // lane 0's
  if (lane == 0)
    for (int t = 0; t < a.n_trees && size < a.heap_cap; ++t) heap_push(heap, size, queue_key(INFINITY, (uint32_t)a.roots[t]));
  uint32_t collected = 0, ncand = 0, pops = 0;
  int overflow = 0;
  for (uint32_t it = 0; it < a.n_nodes && collected < a.search_k; ++it) {  // a node is popped at most once
    unsigned long long top = 0;
    int have = 0;
    if (lane == 0 && size > 0) {
      top = heap_pop(heap, size);
      have = 1;
    }
    have = __shfl(have, 0, 64);
    if (!have) break;
    const uint32_t node = (uint32_t)__shfl((int)(uint32_t)top, 0, 64);
    const uint32_t bkey = (uint32_t)__shfl((int)(uint32_t)(top >> 32), 0, 64);
    ++pops;
    if (node >= a.n_nodes) break;  // (cannot happen: the forest is validated)
    const int4 nd = a.nodes[node];
    if (nd.x & 1) {  // a leaf: its items through the set
      const int count = nd.z;
      for (int i0 = 0; i0 < count; i0 += 64) {
        const int i = i0 + lane;
        bool fresh = false;
        uint32_t item = 0;
        if (i < count) {
          item = (uint32_t)a.items[(size_t)nd.y + i];
          uint32_t h = item * 0x9e3779b1u;
          h = (h ^ (h >> 15)) & mask;
          for (uint32_t probe = 0; probe < a.table_cap; ++probe) {
            const uint32_t old = atomicCAS(&table[h], EMPTY, item);
            if (old == EMPTY) {
              fresh = true;
              break;
            }
            if (old == item) break;
            h = (h + 1) & mask;
          }
        }
        const unsigned long long vote = __ballot(fresh);
        const uint32_t slot = ncand + (uint32_t)__popcll(vote & ((1ull << lane) - 1ull));
        if (fresh && slot < a.cand_cap) cand[slot] = (int32_t)item;
        ncand += (uint32_t)__popcll(vote);
      }
      collected += (uint32_t)count;
    } else {  // a split: the margin, then two pushes
      half8 v[NP];
      load_pieces<NP>(a.normals + (size_t)nd.w * a.stride, true, pieces, v);
      float acc = 0.0f;
#pragma unroll
      for (int j = 0; j < NP; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc += (float)v[j][e] * qf[j][e];
      acc = wave_sum_f32(acc);
      const float mg = a.l2 ? acc + a.offsets[nd.w] : acc;
      if (lane == 0) {
        if (size + 2 > a.heap_cap) {
          overflow = 1;
        } else {
          const float bound = key2f(bkey), neg = -mg;
          heap_push(heap, size, queue_key(mg < bound ? mg : bound, (uint32_t)nd.z));
          heap_push(heap, size, queue_key(neg < bound ? neg : bound, (uint32_t)nd.y));
        }
      }
      overflow = __shfl(overflow, 0, 64);
      if (overflow) break;
    }
  }
  if (lane == 0) {
    a.flags[q] = overflow;
    a.cnt[q] = overflow ? 0 : (int32_t)min(ncand, a.cand_cap);
    a.pops[q] = (int32_t)pops;
    a.collected[q] = (int32_t)collected;
  }
}

struct ScoreArgs {
  const _Float16 *rows;   // the store, [n][stride]
  const _Float16 *q16;    // [m][stride]
  const int32_t *cand;    // [m][cand_cap]
  const int32_t *cnt;     // [m]
  const uint32_t *rank;   // [n]: a position's rank in (id, position) order
  unsigned long long *keys;  // [m][cand_cap]
  uint32_t n, cand_cap;
  int32_t stride, l2;
};

// grid (queries, waves' blocks): wave v of a query scores candidates v * 4 .. v * 4 + 3, then strides on.  The distance of a
// (query, row) pair is row_score.h's, the re-rank's.
template <int NP>
__global__ __launch_bounds__(256) void score_kernel(ScoreArgs a) {
  const int lane = threadIdx.x & 63, q = blockIdx.x;
  const int wave = blockIdx.y * 4 + (threadIdx.x >> 6), waves = gridDim.y * 4;
  const int pieces = a.stride >> 3;
  const int c = min(max(a.cnt[q], 0), (int)a.cand_cap);
  float qf[NP][8];
  load_query<NP>(a.q16 + (size_t)q * a.stride, pieces, qf);
  const int32_t *cp = a.cand + (size_t)q * a.cand_cap;
  unsigned long long *kp = a.keys + (size_t)q * a.cand_cap;
  for (int i0 = wave * ROWS_IN_FLIGHT; i0 < c; i0 += waves * ROWS_IN_FLIGHT) {
    int64_t pos[ROWS_IN_FLIGHT];
    float dist[ROWS_IN_FLIGHT];
#pragma unroll
    for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
      const int64_t p = i0 + u < c ? (int64_t)cp[i0 + u] : -1;
      pos[u] = p < (int64_t)a.n ? p : -1;
    }
    score_rows<NP>(a.rows, a.stride, pieces, pos, qf, a.l2, dist);
#pragma unroll
    for (int u = 0; u < ROWS_IN_FLIGHT; ++u)
      if (lane == 0 && i0 + u < c)
        kp[i0 + u] = pos[u] >= 0 ? ((unsigned long long)f2key(dist[u]) << 32) | a.rank[pos[u]] : ~0ull;
  }
}

struct SelectArgs {
  const unsigned long long *keys;  // [m][cand_cap]
  const int32_t *cnt;
  const int64_t *ids_sorted;       // [n] ids by rank
  uint32_t cand_cap;
  int32_t k;
  float *out_dist;                 // [m][k]
  int64_t *out_ids;
  int32_t *out_counts;
};

// One workgroup per query: the k smallest keys, ascending.
__global__ __launch_bounds__(256) void select_kernel(SelectArgs a) {
  __shared__ unsigned long long keys[SELECT_LDS];
  __shared__ uint32_t hist[258];
  __shared__ uint32_t fill;
  const int t = threadIdx.x, q = blockIdx.x;
  const uint32_t c = (uint32_t)min(max(a.cnt[q], 0), (int)a.cand_cap);
  const unsigned long long *kp = a.keys + (size_t)q * a.cand_cap;
  const uint32_t m = min(c, (uint32_t)a.k);
  uint32_t held = c;  // keys that go to LDS
  if (c <= SELECT_LDS) {
    for (uint32_t i = t; i < c; i += 256) keys[i] = ~kp[i];
  } else {
    // the m-th smallest key (m = k <= 1024 < c): 8 radix passes from the top byte; the keys are distinct
    unsigned long long prefix = 0, pmask = 0;
    uint32_t want = m;
    for (int shift = 56; shift >= 0; shift -= 8) {
      for (int i = t; i < 256; i += 256) hist[i] = 0;
      __syncthreads();
      for (uint32_t i = t; i < c; i += 256) {
        const unsigned long long key = kp[i];
        if ((key & pmask) == prefix) atomicAdd(&hist[(uint32_t)(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (t == 0) {
        uint32_t acc = 0;
        int dgt = 0;
        for (; dgt < 255; ++dgt) {
          if (acc + hist[dgt] >= want) break;
          acc += hist[dgt];
        }
        hist[256] = (uint32_t)dgt;
        hist[257] = want - acc;
      }
      __syncthreads();
      prefix |= (unsigned long long)hist[256] << shift;
      pmask |= 255ull << shift;
      want = hist[257];
      __syncthreads();
    }
    if (t == 0) fill = 0;
    __syncthreads();
    for (uint32_t i = t; i < c; i += 256) {
      const unsigned long long key = kp[i];
      if (key <= prefix) {
        const uint32_t s = atomicAdd(&fill, 1u);
        if (s < SELECT_LDS) keys[s] = ~key;
      }
    }
    __syncthreads();
    held = min(fill, (uint32_t)SELECT_LDS);
  }
  uint32_t n2 = 64;
  while (n2 < held) n2 <<= 1;
  __syncthreads();
  for (uint32_t i = held + t; i < n2; i += 256) keys[i] = 0;  // the complement of the largest key: sorts last
  __syncthreads();
  sort_keys_desc(keys, n2);
  emit_sorted(keys, m, a.k, a.ids_sorted, a.out_dist + (size_t)q * a.k, a.out_ids + (size_t)q * a.k, a.out_counts + q);
}

}  // namespace

struct annoy_index {
  int device = 0;
  annoy_forest forest;  // the index's own copy
  int64_t n = 0;
  int d = 0, stride = 0, metric = 0;
  Buf nodes, normals, offsets, roots, items, rows, rank, ids_sorted;
  // a search
  Buf q16, heap, heap2, table, cand, keys, qlist, cnt, pops, collected, flags, o_dist, o_ids, o_cnt;
  std::vector<int32_t> h_pops, h_collected, h_cnt;
  int64_t first_queue = 0, budget = 0;  // 0: the defaults
  int32_t last_nq = 0, last_width = 0, last_rerun = 0, last_slices = 0;
  bool last_kept = false;
  float t_walk = 0, t_score = 0, t_select = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  ~annoy_index() {
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace {

template <class T>
int upload(Buf &b, const T *src, size_t count) {
  ATRY(b.reserve(count * sizeof(T)));
  if (count) ATRY(hipMemcpy(b.p, src, count * sizeof(T), hipMemcpyHostToDevice));
  return IVF_OK;
}

int from_forest(int32_t device, const annoy_forest_t *forest, const float *rows_fp32, const int64_t *ids, annoy_index_t **out) {
  if (!forest || !rows_fp32 || !out) return fail(IVF_EINVAL, "null argument");
  if (device < 0) return fail(IVF_EINVAL, "device must not be negative");
  const annoy_forest &f = *forest;
  const int64_t n = f.n, n_nodes = f.n_nodes();
  const int d = f.d, stride = f.stride;
  // everything the host prepares, before any device call
  std::vector<uint16_t> rows16((size_t)n * stride);
  if (!annoy_host::prepare_rows(f.metric, d, n, rows_fp32, rows16.data(), stride)) return fail(IVF_EINVAL, "a row component is not finite");
  std::vector<int4> nodes((size_t)n_nodes);
  std::vector<uint16_t> normals((size_t)f.n_splits() * stride, 0);
  int64_t s = 0;
  for (int64_t v = 0; v < n_nodes; ++v) {
    const int32_t *nd = &f.nodes[(size_t)v * 4];
    const bool leaf = nd[0] == ANNOY_NODE_LEAF;
    nodes[(size_t)v] = make_int4((leaf ? 1 : 0) | (nd[3] << 1), nd[1], nd[2], leaf ? -1 : (int32_t)s);
    if (!leaf) {
      std::memcpy(&normals[(size_t)s * stride], &f.normals[(size_t)s * d], (size_t)d * sizeof(uint16_t));
      ++s;
    }
  }
  std::vector<uint32_t> rank((size_t)n);
  std::vector<int64_t> ids_sorted((size_t)n);
  if (ids) {
    std::vector<uint32_t> order((size_t)n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return ids[x] < ids[y]; });
    for (int64_t r = 0; r < n; ++r) {
      rank[order[(size_t)r]] = (uint32_t)r;
      ids_sorted[(size_t)r] = ids[order[(size_t)r]];
    }
  } else {
    for (int64_t r = 0; r < n; ++r) {
      rank[(size_t)r] = (uint32_t)r;
      ids_sorted[(size_t)r] = r + 1;
    }
  }
  std::unique_ptr<annoy_index> ix(new annoy_index);
  ix->forest = f;
  ix->device = device;
  ix->n = n;
  ix->d = d;
  ix->stride = stride;
  ix->metric = f.metric;
  ATRY(hipSetDevice(device));
  for (auto &e : ix->ev) ATRY(hipEventCreate(&e));
  if (int rc = upload(ix->nodes, nodes.data(), nodes.size())) return rc;
  if (int rc = upload(ix->normals, normals.data(), normals.size())) return rc;
  if (int rc = upload(ix->offsets, f.offsets.data(), f.offsets.size())) return rc;
  if (int rc = upload(ix->roots, f.roots.data(), f.roots.size())) return rc;
  if (int rc = upload(ix->items, f.items.data(), f.items.size())) return rc;
  if (int rc = upload(ix->rows, rows16.data(), rows16.size())) return rc;
  if (int rc = upload(ix->rank, rank.data(), rank.size())) return rc;
  if (int rc = upload(ix->ids_sorted, ids_sorted.data(), ids_sorted.size())) return rc;
  *out = ix.release();
  return IVF_OK;
}

// search_k of the header; false if it exceeds the limit
bool effective_search_k(int32_t n_trees, int32_t k, int32_t nodes_to_explore, int64_t *search_k) {
  const int64_t per_tree = std::max<int64_t>(k, nodes_to_explore < 0 ? k : nodes_to_explore / n_trees);
  *search_k = per_tree * n_trees;
  return *search_k <= ANNOY_MAX_SEARCH_K;
}

void launch_walk(const annoy_index *ix, const WalkArgs &a) {
  const dim3 grid((unsigned)((a.m + 3) / 4));
  if (ix->stride <= 512) hipLaunchKernelGGL(walk_kernel<1>, grid, dim3(256), 0, 0, a);
  else hipLaunchKernelGGL(walk_kernel<2>, grid, dim3(256), 0, 0, a);
}

int search(annoy_index_t *ix, int32_t nq, const float *queries, int32_t k, int64_t search_k, float *out_dist, int64_t *out_ids,
           int32_t *out_counts) {
  const annoy_forest &f = ix->forest;
  const int d = ix->d, stride = ix->stride;
  const int64_t n_nodes = f.n_nodes();
  // the prepared queries, on the host as the rows were: the same function, the same bits
  std::vector<uint16_t> q16((size_t)nq * stride);
  if (!annoy_host::prepare_rows(ix->metric, d, nq, queries, q16.data(), stride)) return fail(IVF_EINVAL, "a query component is not finite");
  // the shape of the scratch
  const int64_t cand_cap = std::min<int64_t>(ix->n, search_k - 1 + f.max_leaf);  // fewer than search_k before the last leaf
  int64_t table_cap = 64;
  while (table_cap < 2 * cand_cap) table_cap <<= 1;
  const int64_t heap_cap = std::max<int64_t>(f.n_trees, std::min<int64_t>(n_nodes, ix->first_queue ? ix->first_queue : f.n_trees + DEFAULT_QUEUE));
  const int64_t budget = ix->budget ? ix->budget : DEFAULT_BUDGET;
  const bool keep = (int64_t)nq * cand_cap * 4 <= KEEP_CANDIDATES;  // then the lists of the whole batch stay for the export
  const int64_t per_query = heap_cap * 8 + table_cap * 4 + cand_cap * 8 + (keep ? 0 : cand_cap * 4);
  const int64_t slice = std::max<int64_t>(1, std::min<int64_t>(nq, budget / per_query));
  const int64_t rerun_group = std::max<int64_t>(1, std::min<int64_t>(slice, budget / (n_nodes * 8)));

  ATRY(hipSetDevice(ix->device));
  ix->last_nq = 0;
  ix->last_rerun = ix->last_slices = 0;
  ix->t_walk = ix->t_score = ix->t_select = 0;
  ATRY(ix->q16.reserve(q16.size() * sizeof(uint16_t)));
  ATRY(ix->heap.reserve((size_t)(slice * heap_cap) * 8));
  ATRY(ix->table.reserve((size_t)(slice * table_cap) * 4));
  ATRY(ix->cand.reserve((size_t)((keep ? nq : slice) * cand_cap) * 4));
  ATRY(ix->keys.reserve((size_t)(slice * cand_cap) * 8));
  ATRY(ix->qlist.reserve((size_t)slice * 4));
  for (Buf *b : {&ix->cnt, &ix->pops, &ix->collected, &ix->flags, &ix->o_cnt}) ATRY(b->reserve((size_t)nq * 4));
  ATRY(ix->o_dist.reserve((size_t)nq * k * sizeof(float)));
  ATRY(ix->o_ids.reserve((size_t)nq * k * sizeof(int64_t)));
  ATRY(hipMemcpy(ix->q16.p, q16.data(), q16.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  std::vector<int32_t> flags((size_t)slice), again;

  for (int64_t q0 = 0; q0 < nq; q0 += slice) {
    const int32_t m = (int32_t)std::min<int64_t>(slice, nq - q0);
    WalkArgs w;
    w.nodes = ix->nodes.as<int4>();
    w.normals = ix->normals.as<_Float16>();
    w.offsets = ix->offsets.as<float>();
    w.roots = ix->roots.as<int32_t>();
    w.items = ix->items.as<int32_t>();
    w.q16 = ix->q16.as<_Float16>() + (size_t)q0 * stride;
    w.qlist = nullptr;
    w.heap = ix->heap.as<unsigned long long>();
    w.table = ix->table.as<uint32_t>();
    w.cand = ix->cand.as<int32_t>() + (keep ? (size_t)q0 * cand_cap : 0);
    w.cnt = ix->cnt.as<int32_t>() + q0;
    w.pops = ix->pops.as<int32_t>() + q0;
    w.collected = ix->collected.as<int32_t>() + q0;
    w.flags = ix->flags.as<int32_t>() + q0;
    w.n_nodes = (uint32_t)n_nodes;
    w.heap_cap = (uint32_t)heap_cap;
    w.table_cap = (uint32_t)table_cap;
    w.cand_cap = (uint32_t)cand_cap;
    w.search_k = (uint32_t)search_k;
    w.m = m;
    w.n_trees = f.n_trees;
    w.stride = stride;
    w.l2 = ix->metric == IVF_METRIC_L2;
    ATRY(hipEventRecord(ix->ev[0], 0));
    ATRY(hipMemsetAsync(w.table, 0xff, (size_t)m * table_cap * 4, 0));
    launch_walk(ix, w);
    ATRY(hipGetLastError());
    ATRY(hipMemcpy(flags.data(), w.flags, (size_t)m * 4, hipMemcpyDeviceToHost));
    again.clear();
    for (int32_t i = 0; i < m; ++i)
      if (flags[(size_t)i]) again.push_back(i);
    if (!again.empty() && heap_cap < n_nodes) {  // the second launch: room for every node
      ATRY(ix->heap2.reserve((size_t)(rerun_group * n_nodes) * 8));
      for (size_t g0 = 0; g0 < again.size(); g0 += (size_t)rerun_group) {
        const int32_t gm = (int32_t)std::min<size_t>((size_t)rerun_group, again.size() - g0);
        for (int32_t i = 0; i < gm; ++i)
          ATRY(hipMemsetAsync(w.table + (size_t)again[g0 + i] * table_cap, 0xff, (size_t)table_cap * 4, 0));
        ATRY(hipMemcpy(ix->qlist.p, &again[g0], (size_t)gm * 4, hipMemcpyHostToDevice));
        WalkArgs w2 = w;
        w2.qlist = ix->qlist.as<int32_t>();
        w2.heap = ix->heap2.as<unsigned long long>();
        w2.heap_cap = (uint32_t)n_nodes;
        w2.m = gm;
        launch_walk(ix, w2);
        ATRY(hipGetLastError());
        ATRY(hipStreamSynchronize(0));  // (the list is overwritten by the next group)
      }
      ix->last_rerun += (int32_t)again.size();
    }
    ATRY(hipEventRecord(ix->ev[1], 0));
    ScoreArgs s;
    s.rows = ix->rows.as<_Float16>();
    s.q16 = w.q16;
    s.cand = w.cand;
    s.cnt = w.cnt;
    s.rank = ix->rank.as<uint32_t>();
    s.keys = ix->keys.as<unsigned long long>();
    s.n = (uint32_t)ix->n;
    s.cand_cap = (uint32_t)cand_cap;
    s.stride = stride;
    s.l2 = w.l2;
    const dim3 sgrid((unsigned)m, (unsigned)std::max<int64_t>(1, std::min<int64_t>(32, (cand_cap + 63) / 64)));
    if (stride <= 512) hipLaunchKernelGGL(score_kernel<1>, sgrid, dim3(256), 0, 0, s);
    else hipLaunchKernelGGL(score_kernel<2>, sgrid, dim3(256), 0, 0, s);
    ATRY(hipGetLastError());
    ATRY(hipEventRecord(ix->ev[2], 0));
    SelectArgs e;
    e.keys = s.keys;
    e.cnt = w.cnt;
    e.ids_sorted = ix->ids_sorted.as<int64_t>();
    e.cand_cap = (uint32_t)cand_cap;
    e.k = k;
    e.out_dist = ix->o_dist.as<float>() + (size_t)q0 * k;
    e.out_ids = ix->o_ids.as<int64_t>() + (size_t)q0 * k;
    e.out_counts = ix->o_cnt.as<int32_t>() + q0;
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)m), dim3(256), 0, 0, e);
    ATRY(hipGetLastError());
    ATRY(hipEventRecord(ix->ev[3], 0));
    ATRY(hipStreamSynchronize(0));
    float ms[3] = {0, 0, 0};
    for (int i = 0; i < 3; ++i) (void)hipEventElapsedTime(&ms[i], ix->ev[i], ix->ev[i + 1]);
    ix->t_walk += ms[0];
    ix->t_score += ms[1];
    ix->t_select += ms[2];
    ++ix->last_slices;
  }
  ATRY(hipMemcpy(out_dist, ix->o_dist.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost));
  ATRY(hipMemcpy(out_ids, ix->o_ids.p, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost));
  ATRY(hipMemcpy(out_counts, ix->o_cnt.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
  ix->h_pops.resize((size_t)nq);
  ix->h_collected.resize((size_t)nq);
  ix->h_cnt.resize((size_t)nq);
  ATRY(hipMemcpy(ix->h_pops.data(), ix->pops.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
  ATRY(hipMemcpy(ix->h_collected.data(), ix->collected.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
  ATRY(hipMemcpy(ix->h_cnt.data(), ix->cnt.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
  ix->last_nq = nq;
  ix->last_width = (int32_t)cand_cap;
  ix->last_kept = keep;
  return IVF_OK;
}

}  // namespace

extern "C" {

int annoy_index_from_forest(int32_t device, const annoy_forest_t *forest, const float *rows_fp32, const int64_t *ids,
                            annoy_index_t **out) try {
  return from_forest(device, forest, rows_fp32, ids, out);
} ABI_CATCH

int annoy_index_build(int32_t device, int32_t metric, int32_t d, int64_t n, const float *rows_fp32, const int64_t *ids,
                      int32_t n_trees, int32_t leaf_size, uint64_t seed, int32_t threads, annoy_index_t **out) try {
  if (!out) return fail(IVF_EINVAL, "null argument");
  if (device < 0) return fail(IVF_EINVAL, "device must not be negative");
  annoy_forest_t *f = nullptr;
  if (int rc = annoy_forest_build(metric, d, n, rows_fp32, n_trees, leaf_size, seed, threads, &f)) return rc;
  std::unique_ptr<annoy_forest> hold(f);
  return from_forest(device, f, rows_fp32, ids, out);
} ABI_CATCH

int annoy_search(annoy_index_t *ix, int32_t nq, const float *queries, int32_t k, int32_t nodes_to_explore, float *out_dist,
                 int64_t *out_ids, int32_t *out_counts) try {
  // (the numbers are refused before the handle is looked at)
  if (nq < 1) return fail(IVF_EINVAL, "nq must be positive");
  if (k < 1) return fail(IVF_EINVAL, "k must be positive");
  if (k > ANNOY_MAX_K) return fail(IVF_ELIMIT, "k exceeds 1024");
  if (nodes_to_explore < -1) return fail(IVF_EINVAL, "nodes_to_explore must be -1 (none) or not negative");
  if (!ix || !queries || !out_dist || !out_ids || !out_counts) return fail(IVF_EINVAL, "null argument");
  int64_t search_k = 0;
  if (!effective_search_k(ix->forest.n_trees, k, nodes_to_explore, &search_k))
    return fail(IVF_ELIMIT, "search_k = " + std::to_string(search_k) + " exceeds 262144");
  return search(ix, nq, queries, k, search_k, out_dist, out_ids, out_counts);
} ABI_CATCH

int annoy_index_info(const annoy_index_t *ix, int64_t *n, int32_t *d, int32_t *metric, int32_t *n_trees, int32_t *leaf_size,
                     int64_t *n_nodes) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (n) *n = ix->n;
  if (d) *d = ix->d;
  if (metric) *metric = ix->metric;
  if (n_trees) *n_trees = ix->forest.n_trees;
  if (leaf_size) *leaf_size = ix->forest.leaf_size;
  if (n_nodes) *n_nodes = ix->forest.n_nodes();
  return IVF_OK;
} ABI_CATCH

int annoy_index_get_rows(const annoy_index_t *ix, int64_t row0, int64_t m, uint16_t *out) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (row0 < 0 || m < 0 || row0 > ix->n || m > ix->n - row0) return fail(IVF_EINVAL, "rows outside the index");
  if (m == 0) return IVF_OK;
  if (!out) return fail(IVF_EINVAL, "null argument");
  ATRY(hipSetDevice(ix->device));
  const size_t pitch = (size_t)ix->stride * sizeof(uint16_t), width = (size_t)ix->d * sizeof(uint16_t);
  ATRY(hipMemcpy2D(out, width, ix->rows.as<uint16_t>() + (size_t)row0 * ix->stride, pitch, width, (size_t)m, hipMemcpyDeviceToHost));
  return IVF_OK;
} ABI_CATCH

int annoy_index_forest(const annoy_index_t *ix, const annoy_forest_t **out) try {
  if (!ix || !out) return fail(IVF_EINVAL, "null argument");
  *out = &ix->forest;
  return IVF_OK;
} ABI_CATCH

int annoy_last_candidates(const annoy_index_t *ix, int32_t *nq, int32_t *width, int32_t *out_positions, int32_t *out_counts) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (nq) *nq = ix->last_nq;
  if (width) *width = ix->last_nq > 0 ? ix->last_width : 0;
  if (ix->last_nq > 0 && out_counts) std::copy(ix->h_cnt.begin(), ix->h_cnt.end(), out_counts);
  if (ix->last_nq > 0 && out_positions) {
    if (!ix->last_kept) return fail(IVF_ELIMIT, "the candidate lists of a batch this large are not kept");
    ATRY(hipSetDevice(ix->device));
    const size_t w = (size_t)ix->last_width;
    ATRY(hipMemcpy(out_positions, ix->cand.p, (size_t)ix->last_nq * w * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int32_t q = 0; q < ix->last_nq; ++q) {
      int32_t *row = out_positions + (size_t)q * w;
      const size_t c = (size_t)ix->h_cnt[(size_t)q];
      std::sort(row, row + c);
      std::fill(row + c, row + w, -1);
    }
  }
  return IVF_OK;
} ABI_CATCH

int annoy_last_stats(const annoy_index_t *ix, int32_t *out_pops, int32_t *out_collected, int32_t *rerun, int32_t *slices,
                     float *walk_ms, float *score_ms, float *select_ms) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (ix->last_nq > 0 && out_pops) std::copy(ix->h_pops.begin(), ix->h_pops.end(), out_pops);
  if (ix->last_nq > 0 && out_collected) std::copy(ix->h_collected.begin(), ix->h_collected.end(), out_collected);
  if (rerun) *rerun = ix->last_rerun;
  if (slices) *slices = ix->last_slices;
  if (walk_ms) *walk_ms = ix->t_walk;
  if (score_ms) *score_ms = ix->t_score;
  if (select_ms) *select_ms = ix->t_select;
  return IVF_OK;
} ABI_CATCH

int annoy_debug_set_limits(annoy_index_t *ix, int64_t first_queue_capacity, int64_t scratch_budget_bytes) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (first_queue_capacity < 0 || scratch_budget_bytes < 0) return fail(IVF_EINVAL, "a limit is negative");
  if (first_queue_capacity >= (1ll << 31)) return fail(IVF_EINVAL, "the queue capacity must be below 2^31");
  ix->first_queue = first_queue_capacity;
  ix->budget = scratch_budget_bytes;
  return IVF_OK;
} ABI_CATCH

int annoy_index_destroy(annoy_index_t *ix) try {
  if (ix) (void)hipSetDevice(ix->device);
  delete ix;
  return IVF_OK;
} ABI_CATCH

}  // extern "C"
