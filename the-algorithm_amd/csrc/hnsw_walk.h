// hnsw_walk.h -- the walk of the HNSW graph on the device: the steps that the search kernel (below) and the construction
// kernels (hnsw_build_kernels.h) share, each the restatement of one passage of HnswIndex.java, and the search kernel itself.
// The file header of hnsw_ann.hip says how a walk is laid out on a wave and why.  Included once, by hnsw_ann.hip (through
// hnsw_build_kernels.h); everything is file-local.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/hnsw_ann.h"
#include "hnsw_queue.h"

namespace {

constexpr int MAX_D = 512;
constexpr int MAX_M = 32;        // lists of <= 2*MAX_M = 64 neighbours: one lane each
constexpr int MAX_EF = 1024;
constexpr int CCAP_LDS = 1024;          // most candidate-queue entries kept in LDS (the queue's top)
constexpr int WALK_LDS_BYTES = 9 * 1024;  // dynamic LDS of a walk: result queue + candidate-queue top (16 walks per CU with the static 0.5 KB)
constexpr int VLOG_CAP = 1 << 16;       // visited nodes a walk remembers for cleaning up after itself (more: it wipes its whole bitmap)
// (the host's choices among what the kernels take as arguments: read by hnsw_ann.hip only)
constexpr int CCAP_FIRST = 8192;        // global part of the candidate queue, first pass (64 KB per query)
constexpr int CCAP_GLOBAL = 1 << 17;    // ... of the re-run of a query that outgrew it
constexpr int64_t VLOG_MIN_VWORDS = 1 << 18;  // bitmaps of at least 1 MB keep an undo log

// ---- the search kernel's queues: the heap of hnsw_queue.h over KEntry, in stores that read through uni() ---------------------
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
// a value every lane holds alike, as the search kernel (UNI) or a construction kernel reads it
template <bool UNI, class T>
__device__ __forceinline__ T wave_value(T v) {
  if constexpr (UNI) return uni(v);
  else return v;
}

// The result queue of a search walk: an LDS array.
struct LdsQ {
  KEntry *q;
  __device__ __forceinline__ KEntry get(int i) const { return uni(q[i]); }
  __device__ __forceinline__ void set(int i, const KEntry &e) const { q[i] = e; }
};
// The candidate queue of a search walk: entries [0, nl) in LDS, the rest in global memory (see the header of hnsw_ann.hip).
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
__device__ inline void kq_add(KEntry *q, int &n, KEntry x) { heap_add<KeyOrder<MINQ>>(LdsQ{q}, n, x); }
template <bool MINQ>
__device__ inline KEntry kq_poll(KEntry *q, int &n) { return heap_poll<KeyOrder<MINQ>>(LdsQ{q}, n); }
template <bool MINQ>
__device__ inline void hq_add(const HybQ &q, int &n, KEntry x) { heap_add<KeyOrder<MINQ>>(q, n, x); }
template <bool MINQ>
__device__ inline KEntry hq_poll(const HybQ &q, int &n) { return heap_poll<KeyOrder<MINQ>>(q, n); }

// ---- the visited set --------------------------------------------------------------------------------------------------------
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
// the whole bitmap of a construction walk (vwords is a multiple of 256), where no log is kept
__device__ __forceinline__ void visited_wipe(uint32_t *vis, int64_t vwords, int lane) {
  for (int64_t w = (int64_t)lane * 4; w < vwords; w += 256) *(uint4 *)(vis + w) = make_uint4(0u, 0u, 0u, 0u);
  __threadfence_block();
}

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

// ---- the steps of a walk: templates over CH (chunks of 8 halves per lane: dpad / 64) and the kernel's args struct (SearchArgs
//      or BuildArgs: x, dpad, metric).  ul[64] and ud[64] are the wave's LDS lists of nodes and of their distances. ----

// the wave's query: lane j of every group of 8 holds chunks j, j + 8, ... of the row (the search kernel keeps its own copy)
template <int CH>
__device__ __forceinline__ void load_query_row(const _Float16 *row, int lane, float (&qv)[CH][8]) {
  const half8 *qrow = (const half8 *)row;
  const int j = lane & 7;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const half8 v = qrow[j + 8 * c];
#pragma unroll
    for (int e = 0; e < 8; ++e) qv[c][e] = (float)v[e];
  }
}

// distances of nu nodes (ids in nodes[], LDS) to the wave's query; results to dists[] (LDS)
template <int CH, class Args>
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

// bestEntryPointUntilLayer (HnswIndex.java:447-475) from layer `from` down to layer `stop`, which is not searched; nothing
// when from <= stop (:140-142).  descent_list(a, level, node, ul, lane) is the kernel's own lookup: it reads node's list on
// that layer into ul and returns its length (0: no list).  Moves `cur`; returns the number of distances computed.
template <int CH, bool UNI, class Args>
__device__ __forceinline__ unsigned long long greedy_descent(const Args &a, const float (&qv)[CH][8], uint32_t &cur, int from,
                                                             int stop, uint32_t *ul, float *ud, int lane) {
  if (from <= stop) return 0;
  if (lane == 0) ul[0] = cur;
  __syncthreads();
  wave_distances<CH>(a, qv, ul, ud, 1, lane);
  __syncthreads();
  unsigned long long evals = 1;
  float cur_dist = wave_value<UNI>(ud[0]);
  for (int level = from; level > stop; --level) {
    bool changed = true;
    while (changed) {
      changed = false;
      const int cnt = descent_list(a, level, cur, ul, lane);
      __syncthreads();
      if (cnt > 0) {
        wave_distances<CH>(a, qv, ul, ud, cnt, lane);
        __syncthreads();
        evals += (unsigned long long)cnt;
        // `for nn in list: if (d < curDist) take it`: the running strict minimum, in list order
        for (int i = 0; i < cnt; ++i) {
          const float t = wave_value<UNI>(ud[i]);
          if (t < cur_dist) {
            cur_dist = t;
            cur = wave_value<UNI>(ul[i]);
            changed = true;
          }
        }
      }
      __syncthreads();
    }
  }
  return evals;
}

// The start of searchLayerForCandidates(query, entryPoint, ef, level) (HnswIndex.java:571-578): the entry point's distance,
// which is returned for the kernel's offers to its two queues, its mark in the visited set and the first entry of the log.
template <int CH, class Args>
__device__ __forceinline__ float seed_layer_search(const Args &a, const float (&qv)[CH][8], uint32_t cur, uint32_t *vis,
                                                   uint32_t *vlog, int &n_log, uint32_t *ul, float *ud, int lane) {
  if (lane == 0) ul[0] = cur;
  __syncthreads();
  wave_distances<CH>(a, qv, ul, ud, 1, lane);
  __syncthreads();
  if (lane == 0) {
    atomicOr(&vis[cur >> 5], 1u << (cur & 31));
    if (vlog) vlog[0] = cur;
  }
  n_log = 1;
  return ud[0];
}

// The expansion of a candidate (HnswIndex.java:593-599): of its list (row[1 .. cnt]) the neighbours not yet visited, marked
// now, to ul[0 .. nu) in list order and to the undo log; returns nu, with ul written.
__device__ __forceinline__ int expand_unvisited(const uint32_t *row, int cnt, uint32_t *vis, uint32_t *vlog, int &n_log,
                                                uint32_t *ul, int lane) {
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
  return nu;
}

// ---- the search kernel ------------------------------------------------------------------------------------------------------
// the list of a node on an upper layer; a node that does not reach the layer (no slot, or fewer rows) has none
__device__ __forceinline__ int descent_list(const SearchArgs &a, int level, uint32_t node, uint32_t *ul, int lane) {
  int cnt = 0;
  const int us = a.upper_slot[node];
  if (us >= 0) {
    const int rows = a.upper_base[us + 1] - a.upper_base[us];
    if (level <= rows) {
      const uint32_t *row = a.upper_adj + (size_t)(a.upper_base[us] + level - 1) * (a.m + 1);
      cnt = (int)row[0];
      if (lane < cnt) ul[lane] = row[1 + lane];
    }
  }
  return cnt;
}

// dynamic LDS of the kernel: the result queue [ef + 1], then the top of the candidate queue [ccap_lds]
constexpr size_t search_lds_bytes(int ef, int ccap_lds) { return (size_t)(ef + 1 + ccap_lds) * sizeof(KEntry); }

template <int CH>
__global__ __launch_bounds__(64) void hnsw_search_kernel(SearchArgs a) {
  extern __shared__ KEntry dyn_s[];  // search_lds_bytes(ef, ccap_lds)
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

  // load_query_row, written out: with the call in its place the compiler arranges this kernel's code otherwise, and that build
  // measured 3 % slower at 1M x 256 (profiles/README.md, hnsw_walk_steps; profiles/hnsw_walk_steps_bench_first_build_*.jsonl)
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
  unsigned long long n_exp = 0, n_adm = 0;

  // ---- searchKnn (HnswIndex.java:538-553): the descent to layer 0, then searchLayerForCandidates(query, entryPoint,
  //      max(ef, k), 0) (:571-623) ----
  uint32_t cur = a.entry;
  unsigned long long n_dist = greedy_descent<CH, true>(a, qv, cur, a.max_level, 0, ul, ud, lane);
  const int ef = a.ef;
  const KEntry e0{dist_key(uni(seed_layer_search<CH>(a, qv, cur, vis, vlog, n_log, ul, ud, lane))), cur};
  n_dist += 1;
  int cn = 0, wn = 0, peak = 1;
  bool overflow = false;
  hq_add<true>(cq, cn, e0);
  wq[0] = e0;  // (an offer into an empty queue)
  wn = 1;
  float lower = key_dist(uni(wq[0].key));
  __syncthreads();
  while (cn > 0) {
    const KEntry cand = cq.get(0);
    if (key_dist(cand.key) > lower) break;
    (void)hq_poll<true>(cq, cn);
    n_exp += 1;
    const uint32_t *row = a.adj0 + (size_t)cand.node * (a.m0 + 1);
    const int nu = expand_unvisited(row, (int)uni(row[0]), vis, vlog, n_log, ul, lane);
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

// ---- host: launch -----------------------------------------------------------------------------------------------------------
// The kernels are compiled for rows of CH = 1..8 blocks of 64 elements (dpad = 64 * CH, MAX_D = 512): calls f with CH as a
// std::integral_constant, so that f names the instantiation
template <int CH = 1, class F>
void for_chunks(int chunks, F &&f) {
  if constexpr (CH == 8) f(std::integral_constant<int, 8>());
  else if (chunks == CH) f(std::integral_constant<int, CH>());
  else for_chunks<CH + 1>(chunks, f);
}

int launch_search_any(int chunks, int blocks, const SearchArgs &a, hipStream_t st) {
  const size_t lds = search_lds_bytes(a.ef, a.ccap_lds);
  for_chunks(chunks, [&](auto ch) { hipLaunchKernelGGL((hnsw_search_kernel<decltype(ch)::value>), dim3(blocks), dim3(64), lds, st, a); });
  return HNSW_OK;
}

}  // namespace
