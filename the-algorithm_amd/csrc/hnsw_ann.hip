// hnsw_ann.hip -- HNSW graph search, construction, append and update on gfx950 (include/hnsw_ann.h).  Of the graph the host
// keeps the slot and base tables and one "key exists" flag per row of storage (hnsw_graph_host.h); the lists live on the device,
// and an export reads them from there.  The host-only builder is hnsw_host_builder.h; hnsw_queue.h is what it shares with the kernels.
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
#include "hnsw_queue.h"
#define HTRY(expr) HIP_TRY_AS(HNSW_EDEVICE, expr)
#define ABI_CATCH catch (...) { return abi_guard::caught(fail, HNSW_ENOMEM, HNSW_EINTERNAL); }

namespace {

constexpr int MAX_D = 512;
constexpr int MAX_M = 32;        // lists of <= 2*MAX_M = 64 neighbours: one lane each
constexpr int MAX_EF = 1024;
constexpr int CCAP_LDS = 1024;          // most candidate-queue entries kept in LDS (the queue's top)
constexpr int WALK_LDS_BYTES = 9 * 1024;  // dynamic LDS of a walk: result queue + candidate-queue top (16 walks per CU with the static 0.5 KB)
constexpr int CCAP_FIRST = 8192;        // global part of the candidate queue, first pass (64 KB per query)
constexpr int CCAP_GLOBAL = 1 << 17;    // ... of the re-run of a query that outgrew it
constexpr int64_t VLOG_MIN_VWORDS = 1 << 18;  // bitmaps of at least 1 MB keep an undo log
constexpr int VLOG_CAP = 1 << 16;       // visited nodes a walk remembers for cleaning up after itself (more: it wipes its whole bitmap)

// ---- the search kernel's queues -------------------------------------------------------------------------------------
// Entries carry the distance as an integer KEY whose signed order is Float.compare's (floatToIntBits, then the low 31
// bits flipped for negatives: -0.0 < +0.0, NaN -- canonical -- above +inf), so a heap comparison is one integer compare.
struct KEntry {
  int32_t key;
  uint32_t node;
};
__device__ __forceinline__ int32_t dist_key(float f) {
  const int32_t b = float_to_int_bits(f);
  return b ^ ((b >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float key_dist(int32_t k) { return __int_as_float(k ^ ((k >> 31) & 0x7fffffff)); }
template <bool MINQ>
__device__ __forceinline__ bool k_before(int32_t a, int32_t b) {  // comparator(a, b) < 0
  return MINQ ? a < b : a > b;
}
// Every lane of the wave runs the same queue code on the same data, but a value that comes back from LDS or global memory is
// a vector register as far as the compiler can tell, and every loop and branch that depends on it becomes exec-mask
// bookkeeping (s_and_saveexec / s_or / s_andn2 on masks that are always all-ones: ~35 instructions per sift level in the
// round-3 ISA).  v_readfirstlane says what we know -- the value is wave-uniform -- and counters, heap positions and
// comparisons move to scalar registers, branches become plain s_cbranch (~25 per level).  Measured: no change in kernel time
// (25.0 ms either way at beam 800, 1M x 256): the walk is bound by its chain of dependent LDS / memory round trips and by how
// many walks share a SIMD, not by instruction issue.  Kept because the ISA is the one a reader expects.
__device__ __forceinline__ int32_t uni(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ float uni(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ KEntry uni(const KEntry &e) { return KEntry{uni(e.key), uni(e.node)}; }

// The visited set is an n-bit bitmap per walk -- 6.25 MB at 50M vectors -- of which a walk sets a few thousand bits.  Wiping it
// for every walk (a memset of every bitmap per search launch, or the builder's per-layer wipe) was 5 ms of a 4096-query batch
// and a third of the build at 50M.  Instead every walk LOGS the nodes it marks (VLOG_CAP entries) and clears exactly those
// words when it is done, so a bitmap that starts clean -- one memset when the buffer is allocated -- is clean again for the next
// walk in the slot.  A walk that marks more than the log holds wipes its whole bitmap.  Used from 1 MB per bitmap (8M vectors)
// up: below that the wipes are cheap and the log's stores are not (1M vectors: walk kernel 24.0 -> 25.0 ms with the log).
__device__ __forceinline__ void visited_undo(uint32_t *vis, int64_t vwords, const uint32_t *vlog, int n_log, int lane) {
  __threadfence_block();  // (the log was written by other lanes of this wave)
  if (n_log <= VLOG_CAP) {
    for (int i = lane; i < n_log; i += 64) vis[vlog[i] >> 5] = 0u;
  } else {
    for (int64_t w = lane; w < vwords; w += 64) vis[w] = 0u;
  }
  __threadfence_block();
}

// The candidate queue of a walk: entries [0, nl) in LDS, the rest in global memory (see the file header).
struct HybQ {
  KEntry *lds;
  KEntry *glb;
  int nl;
  __device__ __forceinline__ KEntry get(int i) const { return uni(i < nl ? lds[i] : glb[i - nl]); }
  __device__ __forceinline__ void set(int i, const KEntry &e) const {
    if (i < nl) lds[i] = e;
    else glb[i - nl] = e;
  }
};
template <bool MINQ>
__device__ inline void hq_add(const HybQ &q, int &n, KEntry x) {  // PriorityQueue.offer -> siftUpUsingComparator
  int k = n++;
  while (k > 0) {
    const int parent = (k - 1) >> 1;
    const KEntry e = q.get(parent);
    if (!k_before<MINQ>(x.key, e.key)) break;
    q.set(k, e);
    k = parent;
  }
  q.set(k, x);
}
template <bool MINQ>
__device__ inline KEntry hq_poll(const HybQ &q, int &n) {  // PriorityQueue.poll -> siftDownUsingComparator
  const KEntry result = q.get(0);
  const int s = --n;
  if (s > 0) {
    const KEntry x = q.get(s);
    int k = 0;
    const int half = s >> 1;
    while (k < half) {
      int child = 2 * k + 1;
      KEntry c = q.get(child);
      const int right = child + 1;
      if (right < s) {
        const KEntry r = q.get(right);
        if (k_before<MINQ>(r.key, c.key)) {  // comparator(c, r) > 0
          c = r;
          child = right;
        }
      }
      if (!k_before<MINQ>(c.key, x.key)) break;  // comparator(x, c) <= 0
      q.set(k, c);
      k = child;
    }
    q.set(k, x);
  }
  return result;
}
// plain LDS heap (the result queue): the same two operations without the LDS / global split
template <bool MINQ>
__device__ inline void kq_add(KEntry *q, int &n, KEntry x) {
  int k = n++;
  while (k > 0) {
    const int parent = (k - 1) >> 1;
    const KEntry e = uni(q[parent]);
    if (!k_before<MINQ>(x.key, e.key)) break;
    q[k] = e;
    k = parent;
  }
  q[k] = x;
}
template <bool MINQ>
__device__ inline KEntry kq_poll(KEntry *q, int &n) {
  const KEntry result = uni(q[0]);
  const int s = --n;
  if (s > 0) {
    const KEntry x = uni(q[s]);
    int k = 0;
    const int half = s >> 1;
    while (k < half) {
      int child = 2 * k + 1;
      KEntry c = uni(q[child]);
      const int right = child + 1;
      if (right < s) {
        const KEntry r = uni(q[right]);
        if (k_before<MINQ>(r.key, c.key)) {
          c = r;
          child = right;
        }
      }
      if (!k_before<MINQ>(c.key, x.key)) break;
      q[k] = c;
      k = child;
    }
    q[k] = x;
  }
  return result;
}

// ---------------------------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------------------------
typedef _Float16 half8 __attribute__((ext_vector_type(8)));

struct SearchArgs {
  const _Float16 *x;          // [n][dpad]
  const _Float16 *q;          // [nq][dpad] prepared queries
  const uint32_t *adj0;       // [n][m0 + 1]: count, neighbours
  const int32_t *upper_slot;  // [n]: row group of a node with levels >= 1, or -1
  const int32_t *upper_base;  // [n_upper + 1]: first row of the slot; rows = levels 1..top
  const uint32_t *upper_adj;  // [rows][m + 1]
  const int64_t *ids;         // or NULL
  const int32_t *qlist;       // queries of this launch (spill re-run) or NULL = blockIdx
  uint32_t *visited;          // [slots][vwords]: clean when a walk starts, cleaned by the walk when it ends
  uint32_t *vlog;             // [slots][VLOG_CAP]: the nodes the walk marked; NULL = small bitmaps: the host wipes them per launch
  KEntry *gc;                 // candidate-queue tails: [slots][gcap]
  float *out_dist;            // [nq][k]
  int64_t *out_ids;
  int32_t *out_counts;
  int32_t *spill;             // [nq] set when the LDS candidate queue overflowed
  unsigned long long *stats;  // [0] distance evaluations, [1] expansions, [2] largest candidate queue, [3] admissions
  int64_t vwords;
  int32_t dpad, chunks, m, m0, metric, k, ef, max_level;
  int32_t ccap_lds;           // candidate-queue entries in LDS (the top of the heap)
  int32_t gcap;               // ... and in global memory, per slot
  uint32_t entry;
};

// distances of nu nodes (ids in nodes[], LDS) to the wave's query; results to dists[] (LDS)
template <int CH, class Args>  // chunks of 8 halves per lane: dpad / 64; Args = SearchArgs or BuildArgs (x, dpad, metric)
__device__ __forceinline__ void wave_distances(const Args &a, const float (&qv)[CH][8], const uint32_t *nodes,
                                               float *dists, int nu, int lane) {
  const int g = lane >> 3, j = lane & 7;
  for (int base = 0; base < nu; base += 32) {  // up to 4 rounds of 8 vectors in flight
    half8 xv[4][CH];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int idx = base + r * 8 + g;
      if (idx < nu) {
        const half8 *row = (const half8 *)(a.x + (size_t)nodes[idx] * a.dpad);
#pragma unroll
        for (int c = 0; c < CH; ++c) xv[r][c] = row[j + 8 * c];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int idx = base + r * 8 + g;
      float acc = 0.0f;
      if (idx < nu) {
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float xe = (float)xv[r][c][e];
            if (a.metric == HNSW_METRIC_L2) {
              const float t = qv[c][e] - xe;
              acc = acc + t * t;
            } else {
              // one v_fma_mix_f32 (the fp16 operand converted by the instruction) instead of cvt + mul + add -- and the same
              // bits: both factors are fp16 values, so their product (22 significant bits) is exact in fp32 and the fused
              // form rounds once exactly where `acc + q * x` rounds
              acc = __builtin_fmaf(qv[c][e], xe, acc);
            }
          }
      }
      acc = acc + __shfl_xor(acc, 1, 64);
      acc = acc + __shfl_xor(acc, 2, 64);
      acc = acc + __shfl_xor(acc, 4, 64);
      if (idx < nu && j == 0) dists[idx] = finish_distance(a.metric, acc);
    }
  }
}

template <int CH>
__global__ __launch_bounds__(64) void hnsw_search_kernel(SearchArgs a) {
  extern __shared__ KEntry dyn_s[];  // result queue [ef + 1], then the top of the candidate queue [ccap_lds]
  KEntry *wq = dyn_s;
  __shared__ uint32_t ul[64];
  __shared__ float ud[64];
  const int lane = threadIdx.x;
  const int slot = blockIdx.x;
  const int qi = a.qlist ? a.qlist[slot] : slot;
  const HybQ cq{dyn_s + a.ef + 1, a.gc + (size_t)slot * a.gcap, a.ccap_lds};
  const int ccap = a.ccap_lds + a.gcap;
  uint32_t *vis = a.visited + (size_t)slot * a.vwords;
  uint32_t *vlog = a.vlog ? a.vlog + (size_t)slot * VLOG_CAP : nullptr;  // (uniform)
  int n_log = 0;

  float qv[CH][8];
  {
    const half8 *qrow = (const half8 *)(a.q + (size_t)qi * a.dpad);
    const int j = lane & 7;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const half8 v = qrow[j + 8 * c];
#pragma unroll
      for (int e = 0; e < 8; ++e) qv[c][e] = (float)v[e];
    }
  }
  unsigned long long n_dist = 0, n_exp = 0, n_adm = 0;

  // ---- bestEntryPointUntilLayer (HnswIndex.java:447-475) ----
  uint32_t cur = a.entry;
  if (a.max_level > 0) {
    if (lane == 0) ul[0] = cur;
    __syncthreads();
    wave_distances<CH>(a, qv, ul, ud, 1, lane);
    __syncthreads();
    float cur_dist = uni(ud[0]);
    n_dist += 1;
    for (int level = a.max_level; level > 0; --level) {
      bool changed = true;
      while (changed) {
        changed = false;
        int cnt = 0;
        const int us = a.upper_slot[cur];
        if (us >= 0) {
          const int rows = a.upper_base[us + 1] - a.upper_base[us];
          if (level <= rows) {
            const uint32_t *row = a.upper_adj + (size_t)(a.upper_base[us] + level - 1) * (a.m + 1);
            cnt = (int)row[0];
            if (lane < cnt) ul[lane] = row[1 + lane];
          }
        }
        __syncthreads();
        if (cnt > 0) {
          wave_distances<CH>(a, qv, ul, ud, cnt, lane);
          __syncthreads();
          n_dist += cnt;
          // `for nn in list: if (d < curDist) take it`: the running strict minimum, in list order
          for (int i = 0; i < cnt; ++i) {
            const float t = uni(ud[i]);
            if (t < cur_dist) {
              cur_dist = t;
              cur = uni(ul[i]);
              changed = true;
            }
          }
        }
        __syncthreads();
      }
    }
  }

  // ---- searchLayerForCandidates(query, entryPoint, max(ef, k), 0) (HnswIndex.java:571-623) ----
  const int ef = a.ef;
  if (lane == 0) ul[0] = cur;
  __syncthreads();
  wave_distances<CH>(a, qv, ul, ud, 1, lane);
  __syncthreads();
  n_dist += 1;
  int cn = 0, wn = 0, peak = 1;
  bool overflow = false;
  {
    const KEntry e0{dist_key(uni(ud[0])), cur};
    hq_add<true>(cq, cn, e0);
    wq[0] = e0;  // (an offer into an empty queue)
    wn = 1;
    if (lane == 0) {
      atomicOr(&vis[cur >> 5], 1u << (cur & 31));
      if (vlog) vlog[0] = cur;
    }
    n_log = 1;
  }
  float lower = key_dist(uni(wq[0].key));
  __syncthreads();
  while (cn > 0) {
    const KEntry cand = cq.get(0);
    if (key_dist(cand.key) > lower) break;
    (void)hq_poll<true>(cq, cn);
    n_exp += 1;
    const uint32_t *row = a.adj0 + (size_t)cand.node * (a.m0 + 1);
    const int cnt = (int)uni(row[0]);
    uint32_t nn = 0;
    bool fresh = false;
    if (lane < cnt) {
      nn = row[1 + lane];
      const uint32_t bit = 1u << (nn & 31);
      fresh = (atomicOr(&vis[nn >> 5], bit) & bit) == 0;  // visited.contains / visited.add
    }
    const unsigned long long mask = __ballot(fresh);
    const int nu = __popcll(mask);
    if (fresh) {
      const int at = __popcll(mask & ((1ull << lane) - 1));
      ul[at] = nn;  // list order is kept
      if (vlog && n_log + at < VLOG_CAP) vlog[n_log + at] = nn;
    }
    n_log += nu;
    __syncthreads();
    if (nu > 0) {
      wave_distances<CH>(a, qv, ul, ud, nu, lane);
      __syncthreads();
      n_dist += nu;
      // `lower` never rises once the result queue is full, so a neighbour that fails `d < lower` now fails it when its turn
      // comes: one ballot drops those, and the admission loop -- list order kept -- only visits the rest
      unsigned long long live = __ballot(lane < nu && (wn < ef || ud[lane < nu ? lane : 0] < lower));
      while (live) {
        const int i = __builtin_ctzll(live);
        live &= live - 1;
        const float d = uni(ud[i]);
        if (wn < ef || d < lower) {  // (lower is the result queue's head at all times)
          n_adm += 1;
          if (cn >= ccap) {
            overflow = true;
            break;
          }
          const KEntry e{dist_key(d), uni(ul[i])};
          hq_add<true>(cq, cn, e);
          peak = cn > peak ? cn : peak;
          kq_add<false>(wq, wn, e);
          if (wn > ef) (void)kq_poll<false>(wq, wn);
          lower = key_dist(uni(wq[0].key));
        }
      }
    }
    __syncthreads();
    if (overflow) break;
  }
  if (lane == 0) {
    atomicAdd(&a.stats[0], n_dist);
    atomicAdd(&a.stats[1], n_exp);
    atomicAdd(&a.stats[3], n_adm);
    atomicMax(&a.stats[2], (unsigned long long)(overflow ? ccap + 1 : peak));  // largest candidate queue of the launch
  }
  if (vlog) visited_undo(vis, a.vwords, vlog, n_log, lane);
  if (overflow) {
    if (lane == 0) a.spill[qi] = 1;
    return;
  }
  // dequeueAll (descending), reverse, first k (HnswIndex.java:546-549)
  const int found = wn;
  const int m = found < a.k ? found : a.k;
  for (int pos = found - 1; pos >= 0; --pos) {
    const KEntry e = kq_poll<false>(wq, wn);
    if (pos < m && lane == 0) {
      a.out_dist[(size_t)qi * a.k + pos] = key_dist(e.key);
      a.out_ids[(size_t)qi * a.k + pos] = a.ids ? a.ids[e.node] : (int64_t)e.node;
    }
  }
  if (lane == 0) {
    a.out_counts[qi] = m;
    a.spill[qi] = 0;
  }
}

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

// UPD: the wiring of hnsw_index_update (wireConnectionForAllLayers(..., isUpdate = true), HnswIndex.java:328): the item's level
// is top(u); the walk offers u to the candidate queue but not to the result queue (:607-609); the heuristic drops u, which is
// among the candidates when the walk starts at it (:488-491, :505-507); the item's own lists go to a.own, and a layer whose
// heuristic keeps nobody keeps its old list and continues from u (the reference throws at neighbours.get(0), :439)
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
  {
    const half8 *qrow = (const half8 *)(a.x + (size_t)item * a.dpad);
    const int j = lane & 7;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const half8 v = qrow[j + 8 * c];
#pragma unroll
      for (int e = 0; e < 8; ++e) qv[c][e] = (float)v[e];
    }
  }
  // ---- bestEntryPointUntilLayer(entry, item, maxLayer, itemLevel) (:447-475), when itemLevel < maxLayer (:140-142) ----
  uint32_t cur = a.entry;
  if (item_level < a.max_level) {
    if (lane == 0) ul[0] = cur;
    __syncthreads();
    wave_distances<CH>(a, qv, ul, ud, 1, lane);
    __syncthreads();
    if (UPD) n_evals += 1;
    float cur_dist = ud[0];
    for (int level = a.max_level; level > item_level; --level) {
      bool changed = true;
      while (changed) {
        changed = false;
        const uint32_t *row = layer_row(a, level, cur);
        const int cnt = (int)row[0];
        if (lane < cnt) ul[lane] = row[1 + lane];
        __syncthreads();
        if (cnt > 0) {
          wave_distances<CH>(a, qv, ul, ud, cnt, lane);
          __syncthreads();
          if (UPD) n_evals += (unsigned long long)cnt;
          for (int i = 0; i < cnt; ++i) {
            const float d = ud[i];
            if (d < cur_dist) {
              cur_dist = d;
              cur = ul[i];
              changed = true;
            }
          }
        }
        __syncthreads();
      }
    }
  }
  const int ef = a.efc;
  const int top = item_level < a.max_level ? item_level : a.max_level;
  uint64_t *keys = a.keys + (a.pair_off[a.at + t] - a.pair_off[a.at]);
  for (int level = top; level >= 0; --level) {
    // ---- searchLayerForCandidates(item, cur, efConstruction, level) (:571-623, isUpdate = false): a fresh visited set ----
    int n_log = 0;  // (with a log the bitmap is clean: the previous walk of this slot undid its marks)
    if (!vlog) {
      for (int64_t w = (int64_t)lane * 4; w < a.vwords; w += 256) *(uint4 *)(vis + w) = make_uint4(0u, 0u, 0u, 0u);
      __threadfence_block();
    }
    if (lane == 0) ul[0] = cur;
    __syncthreads();
    wave_distances<CH>(a, qv, ul, ud, 1, lane);
    __syncthreads();
    if (UPD) n_evals += 1;
    int cn = 0, wn = 0;
    {
      const HEntry e0{ud[0], cur};
      pq_add<true>(cq, cn, e0);
      pq_add<false>(wq, wn, e0);
      if (lane == 0) {
        atomicOr(&vis[cur >> 5], 1u << (cur & 31));
        if (vlog) vlog[0] = cur;
      }
      n_log = 1;
    }
    float lower = wq[0].dist;
    __syncthreads();
    while (cn > 0) {
      const HEntry cand = cq[0];
      if (cand.dist > lower) break;
      (void)pq_poll<true>(cq, cn);
      const uint32_t *row = layer_row(a, level, cand.node);
      const int cnt = (int)row[0];
      uint32_t nn = 0;
      bool fresh = false;
      if (lane < cnt) {
        nn = row[1 + lane];
        const uint32_t bit = 1u << (nn & 31);
        fresh = (atomicOr(&vis[nn >> 5], bit) & bit) == 0;  // visited.contains / visited.add
      }
      const unsigned long long mask = __ballot(fresh);
      const int nu = __popcll(mask);
      if (fresh) {
        const int at = __popcll(mask & ((1ull << lane) - 1));
        ul[at] = nn;  // list order is kept
        if (vlog && n_log + at < VLOG_CAP) vlog[n_log + at] = nn;
      }
      n_log += nu;
      __syncthreads();
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
    // ---- selectNearestNeighboursByHeuristic(candidates, maxM) (:479-526); the item itself is never among them ----
    int nk = 0;
    if (wn <= a.m) {  // (:488-491) toListWithItem: the queue's ARRAY order
      if (!UPD) {
        if (lane < wn) kept[lane] = wq[lane].node;
        nk = wn;
      } else {  // list.remove(baseElement): the item occurs at most once
        const bool keep = lane < wn && wq[lane].node != item;
        const unsigned long long mk = __ballot(keep);
        if (keep) kept[__popcll(mk & ((1ull << lane) - 1))] = wq[lane].node;
        nk = __popcll(mk);
      }
      __syncthreads();
    } else {
      cn = 0;  // candidates.reverse() (:495): re-offered in array order under the reversed comparator
      for (int i = 0; i < wn; ++i) pq_add<true>(cq, cn, wq[i]);
      __syncthreads();
      while (cn > 0 && nk < a.m) {
        const HEntry c = pq_poll<true>(cq, cn);
        if (UPD && c.node == item) continue;  // (:505-507)
        if (!heuristic_drops<CH>(a, kept, nk, c.node, c.dist, lane, UPD ? &n_evals : nullptr)) {
          if (lane == 0) kept[nk] = c.node;
          nk++;
          __syncthreads();
        }
      }
    }
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
  const int lane = threadIdx.x, g = lane >> 3, j = lane & 7;
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
  for (int r0 = 0; r0 < n; r0 += 8) {  // distances to the base, eight candidates per round
    const int i = r0 + g;
    float d = 0.0f;
    if (i < n) d = group_row_distance<CH>(a, base, t_id[i], j);
    if (i < n && j == 0) t_d[i] = d;
  }
  __syncthreads();
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
  const int lane = threadIdx.x, g = lane >> 3, j = lane & 7;
  const uint32_t t = blockIdx.x;
  const uint32_t item = a.order[a.at + t];
  uint32_t *vis = a.visited + (size_t)t * a.vwords;
  if (!a.vlog) {  // (without the undo log, bitmaps are left dirty by the walks: wipe; with it they are clean)
    for (int64_t w = (int64_t)lane * 4; w < a.vwords; w += 256) *(uint4 *)(vis + w) = make_uint4(0u, 0u, 0u, 0u);
    __threadfence_block();
  }
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
      for (int r0 = 0; r0 < S; r0 += 8) {  // distFnIndex.distance(neigh, cand), eight candidates per round
        const int i = r0 + g;
        float d = 0.0f;
        if (i < S) d = group_row_distance<CH>(a, v, sc[i], j);
        if (i < S && j == 0) sd[i] = d;
      }
      __syncthreads();
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
      int nk = 0;
      if (wn <= M) {  // toListWithItem (array order); v, the base, is not among them
        if (lane < wn) kept[lane] = wq[lane].node;
        nk = wn;
      } else {
        int cn = 0;
        for (int i = 0; i < wn; ++i) pq_add<true>(mq, cn, wq[i]);
        __syncthreads();
        while (cn > 0 && nk < M) {
          const HEntry c = pq_poll<true>(mq, cn);
          if (!heuristic_drops<CH>(a, kept, nk, c.node, c.dist, lane, &n_evals)) {
            if (lane == 0) kept[nk] = c.node;
            nk++;
            __syncthreads();
          }
        }
      }
      __syncthreads();
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

// The kernels are compiled for rows of CH = 1..8 blocks of 64 elements (dpad = 64 * CH, MAX_D = 512): calls f with CH as a
// std::integral_constant, so that f names the instantiation
template <int CH = 1, class F>
void for_chunks(int chunks, F &&f) {
  if constexpr (CH == 8) f(std::integral_constant<int, 8>());
  else if (chunks == CH) f(std::integral_constant<int, CH>());
  else for_chunks<CH + 1>(chunks, f);
}

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

int launch_search_any(int chunks, int blocks, const SearchArgs &a, hipStream_t st) {
  const size_t lds = (size_t)(a.ef + 1 + a.ccap_lds) * sizeof(HEntry);
  for_chunks(chunks, [&](auto ch) { hipLaunchKernelGGL((hnsw_search_kernel<decltype(ch)::value>), dim3(blocks), dim3(64), lds, st, a); });
  return HNSW_OK;
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
  int lds_n = std::max(64, std::min(CCAP_LDS, (int)((WALK_LDS_BYTES - (size_t)(beam + 1) * sizeof(HEntry)) / sizeof(HEntry))));
  if ((size_t)(beam + 1) * sizeof(HEntry) + 64 * sizeof(HEntry) > (size_t)WALK_LDS_BYTES) lds_n = 64;
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
    HTRY(ix->gc.reserve((size_t)batch * gcap * sizeof(HEntry)));
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
