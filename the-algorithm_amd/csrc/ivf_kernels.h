// ivf_kernels.h -- the device side that the two inverted-file indexes (ivf_ann.hip: flat lists; ivfpq_ann.hip:
// product-quantised lists) share: row preparation, the small bookkeeping kernels of list construction and probe inversion,
// and the survivor buffer's arm / refine kernels.  The survivor buffer itself (Survivor, CAP, f2key, wg_kth_largest, the
// select step's sort) comes from survivor_topk.h, which dense_ann.hip shares, and the device buffer Buf from device_buf.h;
// both reach the sources below through this header.  The host code that launches the kernels is ivf_core.h, which
// includes this; opq_ann.hip and refine_ann.hip use the row preparation.  A source includes this once.  Everything is
// file-local.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ivf_ann.h"
#include "ann_by_id_internal.h"
#include "device_buf.h"
#include "survivor_topk.h"

namespace {

constexpr int MAX_NLIST = 65536;
constexpr int MAX_NPROBE = 1024;
constexpr int CHUNK = ann_by_id::DANN_CHUNK;  // queries (or rows to assign) per coarse search
constexpr int CELL_BITS = 17;                 // radix-sort key width of a cell number

struct Group {
  uint32_t cell, p0, count;  // the queries of the group: pairs [p0, p0 + count) of the probe table sorted by cell
};

// ---------------------------------------------------------------------------------------------
// rows (fp32, row-major) -> fp16 rows (row-major) and the sum of squares of the stored halves.  One wave per row; the
// arithmetic of dense_ann.hip's prep_rows_kernel (Cosine: divide by the fp32 norm, then round).
// ---------------------------------------------------------------------------------------------
// The preparation of one row by one wave: x is the row's d fp32 values, wherever they lie; flat / sumsq as below.
__device__ __forceinline__ void store_row(const float *__restrict__ x, int64_t row, int d, int normalise, int lane,
                                          _Float16 *__restrict__ flat, float *__restrict__ sumsq) {
  double ss = 0;
  for (int k = lane; k < d; k += 64) ss += (double)x[k] * (double)x[k];
  ss = wave_sum(ss);
  float norm = 1.0f;
  if (normalise) {
    norm = (float)sqrt(ss);
    if (!(norm > 0.0f)) norm = 1.0f;
  }
  double ss16 = 0;
  for (int k = lane; k < d; k += 64) {
    _Float16 hv = (_Float16)(x[k] / norm);
    float back = (float)hv;
    ss16 += (double)back * (double)back;
    flat[row * d + k] = hv;
  }
  ss16 = wave_sum(ss16);
  if (lane == 0) sumsq[row] = (float)ss16;
}
__global__ void store_rows_kernel(const float *__restrict__ src, int64_t n, int d, int normalise, _Float16 *__restrict__ flat,
                                  float *__restrict__ sumsq) {
  int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (row >= n) return;
  store_row(src + row * d, row, d, normalise, lane, flat, sumsq);
}
// store_rows_kernel over a position list: row i is rows + pos[i] * d (a by-id query's embedding in the store,
// include/faiss_by_id.h).  The row is gathered into LDS with 16-byte loads (d is a multiple of 16 here, hipMalloc's alignment
// does the rest), and from there store_row runs as above: every lane sums the elements lane, lane + 64, ... it sums there, in
// that order, so flat and sumsq are the bytes store_rows_kernel gives for a copy of the row.  256 threads, one wave per row;
// every position is in the store (the resolve step's, compacted).
__global__ __launch_bounds__(256) void store_rows_pos_kernel(const float *__restrict__ rows, const int64_t *__restrict__ pos, int64_t n,
                                                             int d, int normalise, _Float16 *__restrict__ flat,
                                                             float *__restrict__ sumsq) {
  __shared__ __attribute__((aligned(16))) float stage[4][MAX_D];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + w;
  float *x = stage[w];
  if (row < n) {
    const float4 *s4 = (const float4 *)(rows + pos[row] * d);
    for (int c = lane; c < (d >> 2); c += 64) ((float4 *)x)[c] = s4[c];
  }
  __syncthreads();
  if (row >= n) return;
  store_row(x, row, d, normalise, lane, flat, sumsq);
}

// fp16 rows -> the B-operand fragments of a query chunk: the coarse search's (S_c k-steps, zeroed by dann_chunk_open) and,
// with own != NULL, the scan's (S = d / 16).  One thread per (row, 8-half piece).
__global__ void frag_rows_kernel(const _Float16 *__restrict__ flat, const float *__restrict__ sumsq, int m, int d, int S_c,
                                 _Float16 *__restrict__ qf_c, float *__restrict__ qsumsq, _Float16 *__restrict__ own) {
  const int pieces = d >> 3;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)m * pieces) return;
  const int row = (int)(e / pieces), c = (int)(e % pieces);
  const half8 v = *(const half8 *)&flat[(size_t)row * d + c * 8];
  const int g = row >> 5, r = row & 31, s = c >> 1, h = c & 1;
  *(half8 *)&qf_c[((((size_t)g * S_c + s) * 64) + h * 32 + r) * 8] = v;
  if (own) *(half8 *)&own[((((size_t)g * (d >> 4) + s) * 64) + h * 32 + r) * 8] = v;
  if (c == 0) qsumsq[row] = sumsq[row];
}

__global__ void iota_kernel(uint32_t *__restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (uint32_t)i;
}
__global__ void iota64_kernel(int64_t *__restrict__ out, int64_t first, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = first + i;
}
// the coarse search's answer (k = 1) -> the cell of each row
__global__ void cells_kernel(const int64_t *__restrict__ ids, int m, int32_t *__restrict__ cell) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) cell[i] = (int32_t)ids[i];
}
__global__ void gather_cells_kernel(const int32_t *__restrict__ cell, const uint32_t *__restrict__ perm, int64_t n,
                                    uint32_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (uint32_t)cell[perm ? perm[i] : i];
}
__global__ void hist_kernel(const uint32_t *__restrict__ keys, int64_t n, uint32_t *__restrict__ hist) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) atomicAdd(&hist[keys[i]], 1u);
}
// the blocks of `per` entries that each of n sizes fills
__global__ void blocks_of_kernel(const uint32_t *__restrict__ sizes, int n, uint32_t per, uint32_t *__restrict__ nblk) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) nblk[i] = (sizes[i] + per - 1u) / per;
}

__global__ void fill_kernel(float *__restrict__ p, int64_t n, float v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// ---------------------------------------------------------------------------------------------
// k-means
// ---------------------------------------------------------------------------------------------
__global__ void pick_rows_kernel(const _Float16 *__restrict__ flat, const int64_t *__restrict__ picks, int nlist, int d,
                                 float *__restrict__ cent) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)nlist * d) return;
  cent[e] = (float)flat[(size_t)picks[e / d] * d + e % d];
}
// InnerProduct: the initial picks scaled to unit length, as every later centroid is.  One wave per centroid.
__global__ void unit_rows_kernel(float *__restrict__ cent, int nlist, int d) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= nlist) return;
  float *x = cent + (size_t)row * d;
  double ss = 0;
  for (int k = lane; k < d; k += 64) ss += (double)x[k] * (double)x[k];
  ss = wave_sum(ss);
  if (!(ss > 0)) return;
  const double scale = 1.0 / sqrt(ss);
  for (int k = lane; k < d; k += 64) x[k] = (float)((double)x[k] * scale);
}

// ---------------------------------------------------------------------------------------------
// probe inversion
// ---------------------------------------------------------------------------------------------
// the coarse search's answer [m][nprobe] -> the probe export, the (cell, query) pairs and the number of queries per cell
__global__ void probes_kernel(const int64_t *__restrict__ ids, int m, int nprobe, int32_t *__restrict__ probes,
                              uint32_t *__restrict__ pair_cell, uint32_t *__restrict__ pair_q, uint32_t *__restrict__ per_cell) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)m * nprobe) return;
  const uint32_t c = (uint32_t)ids[e];
  probes[e] = (int32_t)c;
  pair_cell[e] = c;
  pair_q[e] = (uint32_t)(e / nprobe);
  atomicAdd(&per_cell[c], 1u);
}
// ---------------------------------------------------------------------------------------------
// the HNSW coarse quantizer (include/ivf_hnsw_quantizer.h): the graph over the centroids is walked instead of scanned
// ---------------------------------------------------------------------------------------------
// fp16 rows [m][d] -> the prepared-query rows of the graph, [m][dpad] with the padding zeroed: what hnsw_search prepares
// from the same values (L2 and InnerProduct round an fp16 value to itself).  One thread per (row, 8-half piece); d is a
// multiple of 16, so a piece lies inside the row or in the padding.
__global__ void hq_rows_kernel(const _Float16 *__restrict__ flat, int m, int d, int dpad, _Float16 *__restrict__ q) {
  const int pieces = dpad >> 3;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)m * pieces) return;
  const int row = (int)(e / pieces), c = (int)(e % pieces);
  half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
  if (c * 8 < d) v = *(const half8 *)&flat[(size_t)row * d + c * 8];
  *(half8 *)&q[(size_t)row * dpad + c * 8] = v;
}
// probes_kernel for a walk's answer, which may be short: ids [m][nprobe] with counts[q] of them found.  A probe the walk
// did not find is exported as -1; its pair carries the cell number MAX_NLIST, which sorts behind every cell, is counted
// in no per_cell entry and so is read by no scan.  *missing counts them (an integer: any order gives the sum).
__global__ void hq_probes_kernel(const int64_t *__restrict__ ids, const int32_t *__restrict__ counts, int m, int nprobe,
                                 int32_t *__restrict__ probes, uint32_t *__restrict__ pair_cell, uint32_t *__restrict__ pair_q,
                                 uint32_t *__restrict__ per_cell, uint32_t *__restrict__ missing) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)m * nprobe) return;
  const int q = (int)(e / nprobe), j = (int)(e % nprobe);
  pair_q[e] = (uint32_t)q;
  if (j < counts[q]) {
    const uint32_t c = (uint32_t)ids[e];
    probes[e] = (int32_t)c;
    pair_cell[e] = c;
    atomicAdd(&per_cell[c], 1u);
  } else {
    probes[e] = -1;
    pair_cell[e] = (uint32_t)MAX_NLIST;
    atomicAdd(missing, 1u);
  }
}
// one thread per cell: its groups of <= 32 queries, and its share of the rows scanned (integers: any order gives the sum)
__global__ void groups_kernel(const uint32_t *__restrict__ per_cell, const uint32_t *__restrict__ pstart,
                              const uint32_t *__restrict__ gstart, const uint32_t *__restrict__ sizes, int nlist,
                              Group *__restrict__ groups, unsigned long long *__restrict__ rows_scanned) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nlist) return;
  const uint32_t cnt = per_cell[c];
  if (cnt == 0) return;
  for (uint32_t g = 0; g * 32 < cnt; ++g) groups[gstart[c] + g] = Group{(uint32_t)c, pstart[c] + g * 32, min(32u, cnt - g * 32)};
  atomicAdd(rows_scanned, (unsigned long long)cnt * sizes[c]);
}

// after a scan round: a query whose candidates fitted is finished (tau = +inf); one that overflowed is re-armed with the
// k-th largest buffered score.  flags: 1 = another round, 2 = cannot tighten (more than CAP scores tie at the k-th).
__global__ void refine_kernel(float *__restrict__ tau, uint32_t *__restrict__ cnt, uint32_t *__restrict__ done_cnt,
                              const Survivor *__restrict__ surv, int k, int *__restrict__ flags) {
  __shared__ uint32_t hist[258];
  const int q = blockIdx.x;
  if (done_cnt[q] != 0xffffffffu) return;  // finished in an earlier round
  const uint32_t c = cnt[q];
  if (c <= (uint32_t)CAP) {
    if (threadIdx.x == 0) {
      done_cnt[q] = c;
      tau[q] = INFINITY;
    }
    return;
  }
  const float old = tau[q];
  const float nt = wg_kth_largest(&surv[(size_t)q * CAP].score, CAP, 2, k, hist);
  if (threadIdx.x == 0) {
    if (nt > old) {
      tau[q] = nt;
      cnt[q] = 0;
      atomicOr(&flags[0], 1);
    } else {
      tau[q] = INFINITY;
      atomicOr(&flags[0], 2);
    }
  }
}
__global__ void arm_kernel(float *__restrict__ tau, uint32_t *__restrict__ cnt, uint32_t *__restrict__ done_cnt, int nq) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  tau[q] = -INFINITY;
  cnt[q] = 0;
  done_cnt[q] = 0xffffffffu;
}

inline unsigned blocks_for(int64_t n, int per = 256) { return (unsigned)((n + per - 1) / per); }

}  // namespace
