// survivor_topk.h -- the device side of the survivor buffer, the exact top-k scheme that dense_ann.hip and the inverted-file
// sources (through ivf_kernels.h) share: a scan appends every score at or above a per-query threshold to that query's buffer
// of CAP Survivors, wg_kth_largest tightens the threshold of a query whose buffer overflowed, and the select step sorts the
// survivors as 64-bit keys (f2key of the score above, 0xffffffff - rank below) with sort_keys_desc: (score desc, rank asc),
// the tie order the byte-for-byte goldens rest on.  Each source keeps its own scan, its own arm / refine kernels and its own
// key load and emit around the sort.  A source includes this once; everything is file-local.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float16v __attribute__((ext_vector_type(16)));

constexpr int CAP = 8192;  // survivors kept per query (the limit the DANN_ELIMIT / IVF_ELIMIT messages name)
constexpr int MAX_K = 1024;
constexpr int MAX_D = 512;

struct Survivor {
  float score;
  uint32_t pos;  // dense index: the position in row order; inverted files: the list slot
};

__device__ __forceinline__ uint32_t f2key(float f) {  // order-preserving float -> uint
  uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// k-th largest of n floats (stride in floats), one workgroup, 4 radix passes over an LDS histogram
__device__ float wg_kth_largest(const float *vals, int64_t n, int stride, int k, uint32_t *hist /*[258]*/) {
  uint32_t prefix = 0, mask = 0;
  uint32_t want = (uint32_t)k;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
      uint32_t key = f2key(vals[i * stride]);
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t acc = 0;
      int dgt = 255;
      for (; dgt > 0; --dgt) {
        if (acc + hist[dgt] >= want) break;
        acc += hist[dgt];
      }
      hist[256] = (uint32_t)dgt;
      hist[257] = want - acc;
    }
    __syncthreads();
    prefix |= hist[256] << shift;
    mask |= 255u << shift;
    want = hist[257];
    __syncthreads();
  }
  return key2f(prefix);
}

// the n2 keys (a power of two >= 2) of one workgroup's LDS, descending: a bitonic network, every thread of the workgroup in
// every step.  The keys are written and a barrier passed before the call; it ends on a barrier.
__device__ __forceinline__ void sort_keys_desc(unsigned long long *keys, uint32_t n2) {
  for (uint32_t size = 2; size <= n2; size <<= 1)
    for (uint32_t str = size >> 1; str > 0; str >>= 1) {
      for (uint32_t i = threadIdx.x; i < n2 / 2; i += blockDim.x) {
        uint32_t lo = 2 * i - (i & (str - 1));
        uint32_t hi = lo + str;
        bool desc = (lo & size) == 0;
        unsigned long long x = keys[lo], y = keys[hi];
        if ((x < y) == desc) {
          keys[lo] = y;
          keys[hi] = x;
        }
      }
      __syncthreads();
    }
}

}  // namespace
