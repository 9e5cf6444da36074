// hnsw_queue.h -- what the host builder (hnsw_host_builder.h) and the construction kernels (hnsw_ann.hip) share: Float.compare,
// java.util.PriorityQueue restated (same siftUp / siftDown, so equal distances come out as on the JVM), and the distance from
// the fixed-order sum.  Included once, by hnsw_ann.hip; everything is file-local.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../include/hnsw_ann.h"

namespace {

struct HEntry {
  float dist;
  uint32_t node;
};

__host__ __device__ inline int32_t float_to_int_bits(float f) {  // Float.floatToIntBits: canonical NaN
  if (f != f) return 0x7fc00000;
#ifdef __HIP_DEVICE_COMPILE__
  return __float_as_int(f);
#else
  int32_t i;
  std::memcpy(&i, &f, 4);
  return i;
#endif
}
__host__ __device__ inline int float_compare(float a, float b) {  // java.lang.Float.compare
  if (a < b) return -1;
  if (a > b) return 1;
  const int32_t x = float_to_int_bits(a), y = float_to_int_bits(b);
  return x == y ? 0 : (x < y ? -1 : 1);
}
// comparator of a DistancedItemQueue (DistancedItemQueue.java:37-43)
template <bool MINQ>
__host__ __device__ inline int qcmp(const HEntry &a, const HEntry &b) {
  return MINQ ? float_compare(a.dist, b.dist) : float_compare(b.dist, a.dist);
}
// PriorityQueue.offer -> siftUpUsingComparator
template <bool MINQ>
__host__ __device__ inline void pq_add(HEntry *q, int &n, HEntry x) {
  int k = n++;
  while (k > 0) {
    const int parent = (k - 1) >> 1;
    const HEntry e = q[parent];
    if (qcmp<MINQ>(x, e) >= 0) break;
    q[k] = e;
    k = parent;
  }
  q[k] = x;
}
// PriorityQueue.poll -> siftDownUsingComparator
template <bool MINQ>
__host__ __device__ inline HEntry pq_poll(HEntry *q, int &n) {
  const HEntry result = q[0];
  const int s = --n;
  if (s > 0) {
    const HEntry x = q[s];
    int k = 0;
    const int half = s >> 1;
    while (k < half) {
      int child = 2 * k + 1;
      HEntry c = q[child];
      const int right = child + 1;
      if (right < s) {
        const HEntry r = q[right];
        if (qcmp<MINQ>(c, r) > 0) {
          c = r;
          child = right;
        }
      }
      if (qcmp<MINQ>(x, c) <= 0) break;
      q[k] = c;
      k = child;
    }
    q[k] = x;
  }
  return result;
}

// distance from the fixed-order sum (see the header of hnsw_ann.hip)
__host__ __device__ inline float finish_distance(int metric, float s) {
  return metric == HNSW_METRIC_L2 ? sqrtf(s) : 1.0f - s;
}

}  // namespace
