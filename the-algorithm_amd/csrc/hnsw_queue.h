// hnsw_queue.h -- the one binary heap of the HNSW code and what it orders: java.util.PriorityQueue restated (same siftUp /
// siftDown, so equal distances come out as on the JVM), the two entry types with their orders, Float.compare, and the distance
// from the fixed-order sum.  The host builder (hnsw_host_builder.h), the construction kernels (hnsw_build_kernels.h) and the
// search kernel (hnsw_walk.h) all run this heap, each over a store of its own; the stores that need a device intrinsic live
// with the kernels.  Plain C++ without HIP (HNSW_HD is then `inline`), so tests/hnsw_queue_host_check.cpp holds the very
// template against a literal PriorityQueue.  Everything is file-local.
#pragma once
#include <stdint.h>
#include <string.h>

#include <cmath>

#include "../../include/hnsw_ann.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HNSW_HD __host__ __device__ inline
#else
#define HNSW_HD inline
#endif

namespace {

HNSW_HD int32_t float_to_int_bits(float f) {  // Float.floatToIntBits: canonical NaN
  if (f != f) return 0x7fc00000;
#ifdef __HIP_DEVICE_COMPILE__
  return __float_as_int(f);
#else
  int32_t i;
  memcpy(&i, &f, 4);
  return i;
#endif
}
HNSW_HD int float_compare(float a, float b) {  // java.lang.Float.compare
  if (a < b) return -1;
  if (a > b) return 1;
  const int32_t x = float_to_int_bits(a), y = float_to_int_bits(b);
  return x == y ? 0 : (x < y ? -1 : 1);
}

// ---- the entries.  An order's before(a, b) is "comparator(a, b) < 0" of a DistancedItemQueue (DistancedItemQueue.java:37-43),
//      MINQ = nearest first ----
struct HEntry {  // the host builder and the construction kernels: the distance itself, under Float.compare
  float dist;
  uint32_t node;
};
template <bool MINQ>
struct DistOrder {
  static HNSW_HD bool before(const HEntry &a, const HEntry &b) {
    return (MINQ ? float_compare(a.dist, b.dist) : float_compare(b.dist, a.dist)) < 0;
  }
};
// The search kernel: the distance as an integer KEY whose signed order is Float.compare's (floatToIntBits, then the low 31
// bits flipped for negatives: -0.0 < +0.0, NaN -- canonical -- above +inf), so a heap comparison is one integer compare.
struct KEntry {
  int32_t key;
  uint32_t node;
};
HNSW_HD int32_t dist_key(float f) {
  const int32_t b = float_to_int_bits(f);
  return b ^ ((b >> 31) & 0x7fffffff);
}
HNSW_HD float key_dist(int32_t k) {
  const int32_t b = k ^ ((k >> 31) & 0x7fffffff);
#ifdef __HIP_DEVICE_COMPILE__
  return __int_as_float(b);
#else
  float f;
  memcpy(&f, &b, 4);
  return f;
#endif
}
template <bool MINQ>
struct KeyOrder {
  static HNSW_HD bool before(const KEntry &a, const KEntry &b) { return MINQ ? a.key < b.key : a.key > b.key; }
};

// ---- the heap: n entries of a Store (get(i), set(i, e)) under an Order ----
template <class Order, class Store, class Entry>
HNSW_HD void heap_add(const Store &q, int &n, Entry x) {  // PriorityQueue.offer -> siftUpUsingComparator
  int k = n++;
  while (k > 0) {
    const int parent = (k - 1) >> 1;
    const Entry e = q.get(parent);
    if (!Order::before(x, e)) break;  // comparator(x, e) >= 0
    q.set(k, e);
    k = parent;
  }
  q.set(k, x);
}
template <class Order, class Store>
HNSW_HD auto heap_poll(const Store &q, int &n) -> decltype(q.get(0)) {  // PriorityQueue.poll -> siftDownUsingComparator
  using Entry = decltype(q.get(0));
  const Entry result = q.get(0);
  const int s = --n;
  if (s > 0) {
    const Entry x = q.get(s);
    int k = 0;
    const int half = s >> 1;
    while (k < half) {
      int child = 2 * k + 1;
      Entry c = q.get(child);
      const int right = child + 1;
      if (right < s) {
        const Entry r = q.get(right);
        if (Order::before(r, c)) {  // comparator(c, r) > 0
          c = r;
          child = right;
        }
      }
      if (!Order::before(c, x)) break;  // comparator(x, c) <= 0
      q.set(k, c);
      k = child;
    }
    q.set(k, x);
  }
  return result;
}

// a plain array of entries
template <class Entry>
struct ArrayStore {
  Entry *q;
  HNSW_HD Entry get(int i) const { return q[i]; }
  HNSW_HD void set(int i, const Entry &e) const { q[i] = e; }
};
template <bool MINQ>
HNSW_HD void pq_add(HEntry *q, int &n, HEntry x) { heap_add<DistOrder<MINQ>>(ArrayStore<HEntry>{q}, n, x); }
template <bool MINQ>
HNSW_HD HEntry pq_poll(HEntry *q, int &n) { return heap_poll<DistOrder<MINQ>>(ArrayStore<HEntry>{q}, n); }

// distance from the fixed-order sum (see the header of hnsw_ann.hip)
HNSW_HD float finish_distance(int metric, float s) { return metric == HNSW_METRIC_L2 ? sqrtf(s) : 1.0f - s; }

}  // namespace
