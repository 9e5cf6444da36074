// hnsw_build_kernels.h -- the device code of HNSW construction, append and update, over the walk steps of hnsw_walk.h: the
// insert, back-link and relink kernels with their commits, and the row and key kernels of the host paths.  Included once, by
// hnsw_ann.hip; everything is file-local.
#pragma once
#include "hnsw_walk.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Batched index construction on the device (hnsw_index_build_insert_gpu): every step on the GPU, and deterministic.
//
// The reference inserts one item at a time, and with several writer threads it accepts what that costs: "when using
// concurrent writers we can miss connections that we would otherwise get" (HnswIndex.java:376-380).  The device builder is
// that mode taken wide, with the interleaving FIXED so that two builds of one input give one graph (and so that
// oracle/hnsw_oracle.c can restate it: oracle_hnsw_build_batched, compared entry for entry in tests/test_hnsw_gpu_build_gpu.py):
//   order    items by (level descending, position ascending); the first is the entry point and fixes maxLevel for good
//   rounds   round r inserts the next min(batch, max(1, linked / 8)) items of the order against ONE snapshot of the graph
//   phase A  one wave per item (hnsw_build_insert_kernel): wireConnectionForAllLayers (:137-148) as the reference writes it --
//            bestEntryPointUntilLayer, then per layer searchLayerForCandidates with beam efConstruction,
//            selectNearestNeighboursByHeuristic(candidates, maxM), setConnectionList of the NEW item, neighbours.get(0)
//            as the next layer's entry -- but the back links are only recorded: keys (layer, neighbour, order index)
//   sort     the round's keys (hipcub radix sort): all additions to one (layer, node) become one run, in order-index order
//   phase B  one wave per run (hnsw_build_backlink_kernel): append while the list has room (:414-417), else ONE re-selection
//            by the heuristic over the old list followed by the additions, ascending by (Float.compare distance, position)
//            (:419-427 does it once per addition; a round does it once per node)
// No two waves ever write one list, nothing needs a lock or an atomic, nothing returns to the host between rounds.
// Items of one round do not see each other; the graph is therefore not the sequential one (nor is the reference's with two
// writers).  Two bounds the reference does not have, both counted (hnsw_index_build_stats): the candidate queue of a walk
// holds BUILD_CCAP entries -- when full, entries farther than the current bound (which can never be expanded: the walk
// stops at the first such entry, :589-591) are dropped and the heap is rebuilt in array order; a re-selection sees the first
// LINK_CAP entries of old list + additions.
// Appends (hnsw_index_append) run the same two kernels on a live graph: the rounds continue the schedule from linked = n, and
// the entry point / maxLevel are per round (BuildArgs.entry, max_level), since a new row above maxLevel takes over as the entry
// point once its round is done.
// ---------------------------------------------------------------------------------------------
constexpr int BUILD_EF_MAX = 256;  // efConstruction
constexpr int BUILD_CCAP = 1024;   // candidate-queue entries of a construction walk
constexpr int LINK_CAP = 1024;     // old list + additions a re-selection can see

struct BuildArgs {
  const _Float16 *x;
  uint32_t *adj0;              // [n][m0 + 1], updated in place
  const int32_t *upper_slot;
  const int32_t *upper_base;
  uint32_t *upper_adj;         // [rows][m + 1], updated in place
  const uint32_t *order;       // [n] insertion order
  const int32_t *levels;       // [n]
  const int64_t *pair_off;     // [n + 1] by order index: first key slot of an item ((layers wired) * m slots each)
  uint64_t *keys;              // the round's keys: phase A writes (unsorted buffer), phase B reads (sorted buffer)
  uint32_t *visited;           // [round items][vwords]: clean between walks (visited_undo)
  uint32_t *vlog;              // [round items][VLOG_CAP]; NULL = small bitmaps: a walk wipes its own before it starts
  unsigned long long *bstats;  // [0] additions a re-selection did not see, [1] candidate-queue prunes, [2] candidates dropped after a prune
  int64_t vwords;              // a multiple of 256
  int32_t dpad, metric, m, m0, efc, max_level;
  int32_t ccap;                // candidate-queue entries a walk may hold: BUILD_CCAP (smaller only for tests)
  uint32_t entry, at, count;   // the round = order[at .. at + count)
  uint32_t n_keys;
  // hnsw_index_update only (order = the positions of the updated rows, in request order)
  int32_t *utop;               // [order index] top(u) as the round's relink found it; -1 = no HnswNode(0, u)
  const uint64_t *fmask;       // [order index] layers on which the host holds the key HnswNode(level, u)
  const int64_t *prop_off;     // [order index + 1] first relink-proposal slot of an item ((storage layers) * m0 slots each)
  uint32_t *props;             // [round slot][m0 + 1] relink proposals
  uint64_t *pkeys;             // [round slot] (layer << 58 | v << 27 | slot), ~0 = unused
  uint32_t *own;               // [key slot / m][m + 1] the items' own new lists, committed after the round's walks
  uint32_t n_pkeys;
};

__device__ __forceinline__ uint32_t *layer_row(const BuildArgs &a, int level, uint32_t node) {
  if (level == 0) return a.adj0 + (size_t)node * (a.m0 + 1);
  return a.upper_adj + (size_t)(a.upper_base[a.upper_slot[node]] + level - 1) * (a.m + 1);  // (a node listed on a layer has that layer)
}
// greedy_descent's lookup: a node met on a layer has that layer
__device__ __forceinline__ int descent_list(const BuildArgs &a, int level, uint32_t node, uint32_t *ul, int lane) {
  const uint32_t *row = layer_row(a, level, node);
  const int cnt = (int)row[0];
  if (lane < cnt) ul[lane] = row[1 + lane];
  return cnt;
}

// distance between stored rows ra and rb by the 8 lanes of a group (j = lane & 7), the walk's arithmetic with row ra as the
// query; every lane of the group returns the sum
template <int CH>
__device__ __forceinline__ float group_row_distance(const BuildArgs &a, uint32_t ra, uint32_t rb, int j) {
  const half8 *pa = (const half8 *)(a.x + (size_t)ra * a.dpad), *pb = (const half8 *)(a.x + (size_t)rb * a.dpad);
  float acc = 0.0f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const half8 va = pa[j + 8 * c], vb = pb[j + 8 * c];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float fa = (float)va[e], fb = (float)vb[e];
      if (a.metric == HNSW_METRIC_L2) {
        const float t = fa - fb;
        acc = acc + t * t;
      } else {
        acc = __builtin_fmaf(fa, fb, acc);  // (exact product of two fp16 values: the same bits as acc + fa * fb, see wave_distances)
      }
    }
  }
  acc = acc + __shfl_xor(acc, 1, 64);
  acc = acc + __shfl_xor(acc, 2, 64);
  acc = acc + __shfl_xor(acc, 4, 64);
  return finish_distance(a.metric, acc);
}

// distFnIndex.distance(base, ids[i]) for i < n, eight per round, to out[0 .. n) (both LDS); returns with out written
template <int CH>
__device__ __forceinline__ void distances_from_row(const BuildArgs &a, uint32_t base, const uint32_t *ids, int n, float *out,
                                                   int lane) {
  const int g = lane >> 3, j = lane & 7;
  for (int r0 = 0; r0 < n; r0 += 8) {
    const int i = r0 + g;
    float d = 0.0f;
    if (i < n) d = group_row_distance<CH>(a, base, ids[i], j);
    if (i < n && j == 0) out[i] = d;
  }
  __syncthreads();
}

// `kept` (nk entries) vs candidate c at distance dc from the base: is some kept node closer to c than the base is (:508-519)
// (evals: distances computed, added when not NULL)
template <int CH>
__device__ __forceinline__ bool heuristic_drops(const BuildArgs &a, const uint32_t *kept, int nk, uint32_t c, float dc, int lane,
                                                unsigned long long *evals = nullptr) {
  const int g = lane >> 3, j = lane & 7;
  bool drop = false;
  for (int k0 = 0; k0 < nk && !drop; k0 += 8) {
    const int k = k0 + g;
    bool closer = false;
    if (k < nk) closer = group_row_distance<CH>(a, kept[k], c, j) < dc;
    drop = __ballot(closer) != 0ull;
    if (evals) *evals += (unsigned long long)min(8, nk - k0);
  }
  return drop;
}

// selectNearestNeighboursByHeuristic(candidates, M) (HnswIndex.java:479-526) over the max queue wq of wn candidates: the
// neighbours to kept[], their number returned.  `spare` is room for the reversed queue.  SKIP: the candidates may hold the
// item itself (`skip`, at most once), which is never kept (an update: list.remove(baseElement) :488-491, :505-507).
template <int CH, bool SKIP>
__device__ __forceinline__ int select_from_queue(const BuildArgs &a, const HEntry *wq, int wn, HEntry *spare, int M, uint32_t skip,
                                                 uint32_t *kept, int lane, unsigned long long *evals) {
  int nk = 0;
  if (wn <= M) {  // (:488-491) toListWithItem: the queue's ARRAY order
    const bool keep = lane < wn && !(SKIP && wq[lane].node == skip);
    const unsigned long long mk = __ballot(keep);
    if (keep) kept[__popcll(mk & ((1ull << lane) - 1))] = wq[lane].node;
    nk = __popcll(mk);
  } else {
    int cn = 0;  // candidates.reverse() (:495): re-offered in array order under the reversed comparator
    for (int i = 0; i < wn; ++i) pq_add<true>(spare, cn, wq[i]);
    __syncthreads();
    while (cn > 0 && nk < M) {
      const HEntry c = pq_poll<true>(spare, cn);
      if (SKIP && c.node == skip) continue;
      if (!heuristic_drops<CH>(a, kept, nk, c.node, c.dist, lane, evals)) {
        if (lane == 0) kept[nk] = c.node;
        nk++;
        __syncthreads();
      }
    }
  }
  __syncthreads();
  return nk;
}

// UPD: the wiring of hnsw_index_update (wireConnectionForAllLayers(..., isUpdate = true), HnswIndex.java:328): the item's level
// is top(u); the walk offers u to the candidate queue but not to the result queue (:607-609); the heuristic drops u, which is
// among the candidates when the walk starts at it; the item's own lists go to a.own, and a layer whose heuristic keeps nobody
// keeps its old list and continues from u (the reference throws at neighbours.get(0), :439)
template <int CH, bool UPD>
__global__ __launch_bounds__(64) void hnsw_build_insert_kernel(BuildArgs a) {
  __shared__ HEntry wq[BUILD_EF_MAX + 1];
  __shared__ HEntry cq[BUILD_CCAP];
  __shared__ uint32_t ul[64];
  __shared__ float ud[64];
  __shared__ uint32_t kept[MAX_M];
  const int lane = threadIdx.x;
  const uint32_t t = blockIdx.x;
  const uint32_t item = a.order[a.at + t];
  const int item_level = UPD ? a.utop[a.at + t] : a.levels[item];
  if (UPD && item_level < 0) return;  // not in the graph: the row alone changes
  uint32_t *vis = a.visited + (size_t)t * a.vwords;
  uint32_t *vlog = a.vlog ? a.vlog + (size_t)t * VLOG_CAP : nullptr;  // (uniform)
  unsigned long long n_prune = 0, n_dropped = 0, n_evals = 0, n_empty = 0;

  float qv[CH][8];  // the item's own stored row is the query (distFnIndex, item to item)
  load_query_row<CH>(a.x + (size_t)item * a.dpad, lane, qv);
  // ---- wireConnectionForAllLayers (:137-148): the descent to the item's level, then every layer from there down ----
  uint32_t cur = a.entry;
  const unsigned long long n_descent = greedy_descent<CH, false>(a, qv, cur, a.max_level, item_level, ul, ud, lane);
  if (UPD) n_evals += n_descent;
  const int ef = a.efc;
  const int top = item_level < a.max_level ? item_level : a.max_level;
  uint64_t *keys = a.keys + (a.pair_off[a.at + t] - a.pair_off[a.at]);
  for (int level = top; level >= 0; --level) {
    // ---- searchLayerForCandidates(item, cur, efConstruction, level) (:571-623, isUpdate = false): a fresh visited set ----
    int n_log = 0;  // (with a log the bitmap is clean: the previous walk of this slot undid its marks)
    if (!vlog) visited_wipe(vis, a.vwords, lane);
    const HEntry e0{seed_layer_search<CH>(a, qv, cur, vis, vlog, n_log, ul, ud, lane), cur};
    if (UPD) n_evals += 1;
    int cn = 0, wn = 0;
    pq_add<true>(cq, cn, e0);
    pq_add<false>(wq, wn, e0);
    float lower = wq[0].dist;
    __syncthreads();
    while (cn > 0) {
      const HEntry cand = cq[0];
      if (cand.dist > lower) break;
      (void)pq_poll<true>(cq, cn);
      const uint32_t *row = layer_row(a, level, cand.node);
      const int nu = expand_unvisited(row, (int)row[0], vis, vlog, n_log, ul, lane);
      if (nu > 0) {
        wave_distances<CH>(a, qv, ul, ud, nu, lane);
        __syncthreads();
        if (UPD) n_evals += (unsigned long long)nu;
        for (int i = 0; i < nu; ++i) {
          const HEntry e{ud[i], ul[i]};
          if (wn < ef || e.dist < wq[0].dist) {
            if (cn >= a.ccap) {  // drop what can never be expanded, rebuild the heap in array order
              const int had = cn;
              cn = 0;
              for (int s = 0; s < had; ++s) {
                const HEntry x = cq[s];
                if (!(x.dist > lower)) pq_add<true>(cq, cn, x);
              }
              n_prune += 1;
            }
            if (cn < a.ccap) pq_add<true>(cq, cn, e);
            else n_dropped += 1;
            if (UPD && e.node == item) continue;  // (:607-609)
            pq_add<false>(wq, wn, e);
            if (wn > ef) (void)pq_poll<false>(wq, wn);
            lower = wq[0].dist;
          }
        }
      }
      __syncthreads();
    }
    if (vlog) visited_undo(vis, a.vwords, vlog, n_log, lane);
    // (an insert's item is never among its candidates; an update's is, when the walk starts at it)
    const int nk = select_from_queue<CH, UPD>(a, wq, wn, cq, a.m, item, kept, lane, UPD ? &n_evals : nullptr);
    // ---- setConnectionList(item, level, neighbours) (:393); the back links become keys ----
    uint32_t *row = UPD ? a.own + (size_t)((keys - a.keys) / a.m + (top - level)) * (a.m + 1) : layer_row(a, level, item);
    if (lane < nk) row[1 + lane] = kept[lane];
    if (lane == 0) row[0] = UPD && nk == 0 ? ~0u : (uint32_t)nk;  // (UPD, nobody kept: the old list stays)
    uint64_t *kslot = keys + (size_t)(top - level) * a.m;
    if (lane < a.m)
      kslot[lane] = lane < nk ? ((uint64_t)level << 56) | ((uint64_t)kept[lane] << 24) | (uint64_t)t : ~0ull;
    if (UPD && nk == 0) n_empty += 1;
    cur = UPD && nk == 0 ? item : kept[0];  // neighbours.get(0) (:439)
    __syncthreads();
  }
  if (lane == 0 && (n_prune | n_dropped)) {
    atomicAdd(&a.bstats[1], n_prune);
    atomicAdd(&a.bstats[2], n_dropped);
  }
  if (UPD && lane == 0) {
    atomicAdd(&a.bstats[3], n_empty);
    atomicAdd(&a.bstats[7], n_evals);
  }
}

// UPD: the back links of hnsw_index_update (mutuallyConnectNewElement(..., isUpdate = true)): an addition of an item the list
// already holds is dropped and counted (:405-412); the rest is the builder's phase B
template <int CH, bool UPD>
__global__ __launch_bounds__(64) void hnsw_build_backlink_kernel(BuildArgs a) {
  __shared__ uint32_t t_id[LINK_CAP];
  __shared__ float t_d[LINK_CAP];
  __shared__ uint32_t c_id[LINK_CAP];
  __shared__ float c_d[LINK_CAP];
  __shared__ uint32_t kept[2 * MAX_M];
  const int lane = threadIdx.x;
  const uint32_t i0 = blockIdx.x;
  const uint64_t key = a.keys[i0];
  if (key == ~0ull) return;
  const uint64_t run = key >> 24;  // (layer, node)
  if (i0 > 0 && (a.keys[i0 - 1] >> 24) == run) return;  // not the head of its run
  const int level = (int)(key >> 56);
  const uint32_t base = (uint32_t)(run & 0xffffffffull);
  int add_n = 0;
  for (uint32_t b = i0;; b += 64) {
    const uint32_t idx = b + lane;
    const bool same = idx < a.n_keys && (a.keys[idx] >> 24) == run;
    const unsigned long long mask = __ballot(same);
    if (mask == ~0ull) {
      add_n += 64;
      continue;
    }
    add_n += __builtin_ctzll(~mask);
    break;
  }
  const int M = level == 0 ? a.m0 : a.m;
  uint32_t *row = layer_row(a, level, base);
  const int old_n = (int)row[0];
  if (UPD) {  // old list, then the additions it does not hold yet, into t_id (as far as LINK_CAP)
    for (int i = lane; i < old_n; i += 64) t_id[i] = row[1 + i];
    __syncthreads();
    int kn = 0;
    for (int b0 = 0; b0 < add_n; b0 += 64) {
      const int i = b0 + lane;
      uint32_t it = 0;
      bool keep = false;
      if (i < add_n) {
        it = a.order[a.at + (uint32_t)(a.keys[i0 + i] & 0xffffffull)];
        keep = true;
        for (int e = 0; e < old_n; ++e)
          if (t_id[e] == it) {
            keep = false;
            break;
          }
      }
      const unsigned long long mk = __ballot(keep);
      const int at = old_n + kn + __popcll(mk & ((1ull << lane) - 1));
      if (keep && at < LINK_CAP) t_id[at] = it;
      kn += __popcll(mk);
    }
    __syncthreads();
    if (lane == 0 && kn < add_n) atomicAdd(&a.bstats[6], (unsigned long long)(add_n - kn));
    add_n = kn;
    if (add_n == 0) return;
  }
  if (old_n + add_n <= M) {  // room: append, in order-index order (:414-417)
    for (int i = lane; i < add_n; i += 64)
      row[1 + old_n + i] = UPD ? t_id[old_n + i] : a.order[a.at + (uint32_t)(a.keys[i0 + i] & 0xffffffull)];
    __syncthreads();
    if (lane == 0) row[0] = (uint32_t)(old_n + add_n);
    return;
  }
  int n = old_n + add_n;
  if (n > LINK_CAP) {
    if (lane == 0) atomicAdd(&a.bstats[0], (unsigned long long)(n - LINK_CAP));
    n = LINK_CAP;
  }
  if (!UPD)
    for (int i = lane; i < n; i += 64) t_id[i] = i < old_n ? row[1 + i] : a.order[a.at + (uint32_t)(a.keys[i0 + (i - old_n)] & 0xffffffull)];
  __syncthreads();
  unsigned long long n_evals = (unsigned long long)n;
  distances_from_row<CH>(a, base, t_id, n, t_d, lane);
  for (int i = lane; i < n; i += 64) {  // ascending by (Float.compare distance, position): every lane ranks its candidates by counting
    const float d = t_d[i];
    int rank = 0;
    for (int e = 0; e < n; ++e) {
      const int c = float_compare(t_d[e], d);
      rank += (c < 0 || (c == 0 && e < i)) ? 1 : 0;
    }
    c_id[rank] = t_id[i];
    c_d[rank] = d;
  }
  __syncthreads();
  int nk = 0;  // n > M here: the heuristic proper (:495-523)
  for (int i = 0; i < n && nk < M; ++i) {
    const uint32_t c = c_id[i];
    if (c == base) continue;
    if (!heuristic_drops<CH>(a, kept, nk, c, c_d[i], lane, UPD ? &n_evals : nullptr)) {
      if (lane == 0) kept[nk] = c;
      nk++;
      __syncthreads();
    }
  }
  __syncthreads();
  for (int i = lane; i < nk; i += 64) row[1 + i] = kept[i];
  if (lane == 0) row[0] = (uint32_t)nk;
  if (UPD && lane == 0) atomicAdd(&a.bstats[7], n_evals);
}

// ---- hnsw_index_update: HnswIndex.reInsert (HnswIndex.java:226-329) in rounds (include/hnsw_ann.h) ----
// Per round: the rows (hnsw_update_rows_kernel), the relink proposals against the graph as the round found it
// (hnsw_update_relink_kernel), the latest proposal per (layer, v) committed (hnsw_update_relink_commit_kernel), the wiring
// walks (hnsw_build_insert_kernel<UPD>) with the items' own lists committed after all of them (hnsw_update_own_commit_kernel),
// and the back links (hnsw_build_backlink_kernel<UPD>).
constexpr int SETCAND_MAX = 1 + 2 * MAX_M + 4 * MAX_M * MAX_M;  // u, N_l(u), and N_l(e) for every e: 4161 at maxM = 32

// One wave per round item u.  top(u) (:244-250), then per layer 0..top(u) with a non-empty N_l(u) (:259-262): setCand in
// insertion order -- u, then each e of N_l(u) followed by N_l(e), first occurrence kept (a HashSet in the reference) -- and for
// every v of N_l(u) other than u (updateNeighborProbability = 1, :271) the proposal for v's list: setCand \ {v} offered in
// enumeration order to a max queue of min(efC, |set|) entries (:281-309), then selectNearestNeighboursByHeuristic with maxM0 on
// layer 0, maxM above (:311-314).  The walk's visited bitmap of the slot is the set's membership test; it is clean again after
// every layer.
template <int CH>
__global__ __launch_bounds__(64) void hnsw_update_relink_kernel(BuildArgs a) {
  __shared__ uint32_t sc[SETCAND_MAX];
  __shared__ float sd[SETCAND_MAX];
  __shared__ HEntry wq[BUILD_EF_MAX + 1];
  __shared__ HEntry mq[BUILD_EF_MAX + 1];
  __shared__ uint32_t nl[2 * MAX_M];
  __shared__ uint32_t kept[2 * MAX_M];
  const int lane = threadIdx.x;
  const uint32_t t = blockIdx.x;
  const uint32_t item = a.order[a.at + t];
  uint32_t *vis = a.visited + (size_t)t * a.vwords;
  if (!a.vlog) visited_wipe(vis, a.vwords, lane);  // (without the undo log, bitmaps are left dirty by the walks; with it they are clean)
  // ---- top(u): the highest layer <= maxLevel on which HnswNode(layer, u) exists -- a key the host holds, or a non-empty
  //      row -- and -1 when HnswNode(0, u) does not (the reference's checkState, :239-240) ----
  const uint64_t fm = a.fmask[a.at + t];
  const int32_t slot = a.upper_slot[item];
  const int stor = slot < 0 ? 0 : a.upper_base[slot + 1] - a.upper_base[slot];
  int top = -1;
  if ((fm & 1ull) || a.adj0[(size_t)item * (a.m0 + 1)] > 0) {
    top = 0;
    for (int l = 1; l <= min(stor, a.max_level); ++l)
      if (((fm >> l) & 1ull) || layer_row(a, l, item)[0] > 0) top = l;
  }
  if (lane == 0) a.utop[a.at + t] = top;
  unsigned long long n_relinks = 0, n_evals = 0;
  const int64_t pbase = a.prop_off[a.at + t] - a.prop_off[a.at];
  for (int level = 0; level <= top; ++level) {
    const uint32_t *row = layer_row(a, level, item);
    const int cnt = (int)row[0];
    if (cnt == 0) continue;
    if (lane < cnt) nl[lane] = row[1 + lane];
    if (lane == 0) {
      sc[0] = item;
      atomicOr(&vis[item >> 5], 1u << (item & 31));
    }
    int S = 1;
    __syncthreads();
    for (int e = 0; e < cnt; ++e) {
      const uint32_t el = nl[e];
      bool fresh = false;
      if (lane == 0) {
        const uint32_t bit = 1u << (el & 31);
        fresh = (atomicOr(&vis[el >> 5], bit) & bit) == 0;
        if (fresh) sc[S] = el;
      }
      S += __ballot(fresh) ? 1 : 0;
      const uint32_t *r2 = layer_row(a, level, el);
      const int c2 = (int)r2[0];
      uint32_t nn = 0;
      bool part = lane < c2;
      if (part) nn = r2[1 + lane];
      for (int k = 0; k < 64; ++k) {  // of an id repeated within the list, the first occurrence alone takes part
        const uint32_t o = __shfl(nn, k, 64);
        if (k < lane && k < c2 && o == nn) part = false;
      }
      fresh = false;
      if (part) {
        const uint32_t bit = 1u << (nn & 31);
        fresh = (atomicOr(&vis[nn >> 5], bit) & bit) == 0;
      }
      const unsigned long long mk = __ballot(fresh);
      if (fresh) sc[S + __popcll(mk & ((1ull << lane) - 1))] = nn;
      S += __popcll(mk);
      __syncthreads();
    }
    const int M = level == 0 ? a.m0 : a.m;
    for (int jv = 0; jv < cnt; ++jv) {
      const uint32_t v = nl[jv];
      if (v == item) continue;  // setNeigh.remove(item) (:279)
      distances_from_row<CH>(a, v, sc, S, sd, lane);  // distFnIndex.distance(neigh, cand)
      n_evals += (unsigned long long)S;
      const int keep = min(a.efc, S - 1);  // |setCopy| = |setCand| - 1: v is in the set
      int wn = 0;
      for (int i = 0; i < S; ++i) {
        const uint32_t c = sc[i];
        if (c == v) continue;
        const HEntry e{sd[i], c};
        if (wn < keep) {
          pq_add<false>(wq, wn, e);
        } else if (e.dist < wq[0].dist) {
          (void)pq_poll<false>(wq, wn);
          pq_add<false>(wq, wn, e);
        }
      }
      __syncthreads();
      const int nk = select_from_queue<CH, false>(a, wq, wn, mq, M, 0u, kept, lane, &n_evals);  // (v, the base, is not among them)
      const int64_t ps = pbase + (int64_t)level * a.m0 + jv;
      uint32_t *prow = a.props + (size_t)ps * (a.m0 + 1);
      if (lane < nk) prow[1 + lane] = kept[lane];
      if (lane == 0) {
        prow[0] = (uint32_t)nk;
        a.pkeys[ps] = ((uint64_t)level << 58) | ((uint64_t)v << 27) | (uint64_t)ps;
      }
      n_relinks += 1;
      __syncthreads();
    }
    __threadfence_block();
    for (int i = lane; i < S; i += 64) vis[sc[i] >> 5] = 0u;  // the bitmap clean again
    __threadfence_block();
    __syncthreads();
  }
  if (lane == 0) {
    atomicAdd(&a.bstats[4], n_relinks);
    atomicAdd(&a.bstats[7], n_evals);
  }
}

// pkeys sorted: the last proposal of every (layer, v) run -- the latest item in request order -- is v's new list; the others are
// superseded (a later reInsert overwrites an earlier one's setConnectionList)
__global__ void hnsw_update_relink_commit_kernel(BuildArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)a.n_pkeys) return;
  const uint64_t key = a.pkeys[i];
  if (key == ~0ull) return;
  const uint64_t run = key >> 27;
  if (i + 1 < (int64_t)a.n_pkeys && (a.pkeys[i + 1] >> 27) == run) {
    atomicAdd(&a.bstats[5], 1ull);
    return;
  }
  const int level = (int)(key >> 58);
  const uint32_t v = (uint32_t)(run & 0x7fffffffull);
  const uint32_t *p = a.props + (size_t)(key & ((1ull << 27) - 1)) * (a.m0 + 1);
  uint32_t *row = layer_row(a, level, v);
  const uint32_t c = p[0];
  for (uint32_t k = 0; k < c; ++k) row[1 + k] = p[1 + k];
  row[0] = c;
}

// the items' own lists of the round, once every walk has ended (a layer whose heuristic kept nobody keeps its list)
__global__ __launch_bounds__(64) void hnsw_update_own_commit_kernel(BuildArgs a) {
  const uint32_t t = blockIdx.x;
  const int lane = threadIdx.x;
  const uint32_t item = a.order[a.at + t];
  const int top = a.utop[a.at + t];
  const int64_t kb = (a.pair_off[a.at + t] - a.pair_off[a.at]) / a.m;
  for (int level = 0; level <= top; ++level) {
    const uint32_t *o = a.own + (size_t)(kb + (top - level)) * (a.m + 1);
    const uint32_t c = o[0];
    if (c == ~0u) continue;
    uint32_t *row = layer_row(a, level, item);
    if ((uint32_t)lane < c) row[1 + lane] = o[1 + lane];
    if (lane == 0) row[0] = c;
  }
}

// the round's rows, prepared as at build time (hnsw_prep_rows), into their positions
__global__ void hnsw_update_rows_kernel(const float *__restrict__ src, int64_t n, const uint32_t *__restrict__ pos, int d, int dpad,
                                        int normalise, _Float16 *__restrict__ dst) {
  int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (row >= n) return;
  const float *x = src + row * d;
  float norm = 1.0f;
  if (normalise) {
    double ss = 0;
    for (int k = lane; k < d; k += 64) ss += (double)x[k] * (double)x[k];
    for (int o = 32; o; o >>= 1) ss += __shfl_xor(ss, o, 64);
    norm = (float)sqrt(ss);
    if (!(norm > 0.0f)) norm = 1.0f;
  }
  _Float16 *y = dst + (int64_t)pos[row] * dpad;
  for (int k = lane; k < dpad; k += 64) y[k] = (_Float16)(k < d ? x[k] / norm : 0.0f);
}

// key -> position of a keyed index: the (key, position) table sorted by key, one binary search per requested key (-1: absent)
__global__ void hnsw_key_lookup_kernel(const int64_t *__restrict__ keys, const int64_t *__restrict__ pos, int64_t nt,
                                       const int64_t *__restrict__ q, int64_t nq, int64_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  const int64_t k = q[i];
  int64_t lo = 0, hi = nt;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  out[i] = lo < nt && keys[lo] == k ? pos[lo] : -1;
}
__global__ void hnsw_iota_kernel(int64_t *__restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = i;
}

// ---- host: launch of the CH instantiations (for_chunks, hnsw_walk.h) ----
void launch_update_any(int chunks, const BuildArgs &a, hipStream_t st, int which, unsigned grid) {
  for_chunks(chunks, [&](auto ch) {
    constexpr int CH = decltype(ch)::value;
    if (which == 0) hipLaunchKernelGGL((hnsw_update_relink_kernel<CH>), dim3(grid), dim3(64), 0, st, a);
    else if (which == 1) hipLaunchKernelGGL((hnsw_build_insert_kernel<CH, true>), dim3(grid), dim3(64), 0, st, a);
    else hipLaunchKernelGGL((hnsw_build_backlink_kernel<CH, true>), dim3(grid), dim3(64), 0, st, a);
  });
}

void launch_build_any(int chunks, const BuildArgs &a_ins, const BuildArgs &a_link, hipStream_t st, int which) {
  for_chunks(chunks, [&](auto ch) {
    constexpr int CH = decltype(ch)::value;
    if (which == 0) hipLaunchKernelGGL((hnsw_build_insert_kernel<CH, false>), dim3(a_ins.count), dim3(64), 0, st, a_ins);
    else hipLaunchKernelGGL((hnsw_build_backlink_kernel<CH, false>), dim3(a_link.n_keys), dim3(64), 0, st, a_link);
  });
}

// rows (fp32) -> fp16 rows padded to dpad; Cosine rows are normalised first (Hnsw.scala:149-155)
__global__ void hnsw_prep_rows(const float *__restrict__ src, int64_t n, int d, int dpad, int normalise,
                               _Float16 *__restrict__ dst) {
  int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (row >= n) return;
  const float *x = src + row * d;
  float norm = 1.0f;
  if (normalise) {
    double ss = 0;
    for (int k = lane; k < d; k += 64) ss += (double)x[k] * (double)x[k];
    for (int o = 32; o; o >>= 1) ss += __shfl_xor(ss, o, 64);
    norm = (float)sqrt(ss);
    if (!(norm > 0.0f)) norm = 1.0f;
  }
  for (int k = lane; k < dpad; k += 64) dst[row * dpad + k] = (_Float16)(k < d ? x[k] / norm : 0.0f);
}

__global__ void hnsw_rows_to_f32(const _Float16 *__restrict__ src, int64_t i0, int64_t n, int d, int dpad,
                                 float *__restrict__ dst) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * d) return;
  dst[e] = (float)src[(i0 + e / d) * dpad + e % d];
}

// ---- the keys of an append (hnsw_index_append): IllegalDuplicateInsertException on the device ----
// The index keeps its keys sorted (`table`, nt entries); an append sorts its own keys (`b`, nb entries) and every key looks
// itself up: a repeat of its predecessor in the batch, or a hit in the table, is a duplicate.  The first offending batch
// index (in sorted order) is left in *bad (which starts at INT32_MAX).
__global__ void hnsw_key_probe_kernel(const int64_t *__restrict__ table, int64_t nt, const int64_t *__restrict__ b, int64_t nb,
                                      int32_t *__restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  const int64_t k = b[i];
  bool dup = i > 0 && b[i - 1] == k;
  if (!dup) {
    int64_t lo = 0, hi = nt;  // lower_bound
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (table[mid] < k) lo = mid + 1;
      else hi = mid;
    }
    dup = lo < nt && table[lo] == k;
  }
  if (dup) atomicMin(bad, (int32_t)i);
}

// Merge path: the sorted table and the sorted batch into one sorted table of na + nb keys.  Thread t writes outputs
// [t * MERGE_ITEMS, (t + 1) * MERGE_ITEMS): a binary search along that diagonal finds how many of them come from `a`, then a
// sequential merge of MERGE_ITEMS steps (ties: `a` first; an append that reaches this has no ties).
constexpr int MERGE_ITEMS = 8;
__global__ void hnsw_key_merge_kernel(const int64_t *__restrict__ a, int64_t na, const int64_t *__restrict__ b, int64_t nb,
                                      int64_t *__restrict__ out) {
  const int64_t total = na + nb;
  const int64_t diag = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * MERGE_ITEMS;
  if (diag >= total) return;
  int64_t lo = diag > nb ? diag - nb : 0, hi = diag < na ? diag : na;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] <= b[diag - 1 - mid]) lo = mid + 1;
    else hi = mid;
  }
  int64_t i = lo, j = diag - lo;
  for (int s = 0; s < MERGE_ITEMS && diag + s < total; ++s) {
    const bool take_a = j >= nb || (i < na && a[i] <= b[j]);
    out[diag + s] = take_a ? a[i++] : b[j++];
  }
}

}  // namespace
