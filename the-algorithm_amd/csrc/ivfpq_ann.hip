// ivfpq_ann.hip -- inverted-file index with product-quantised lists (`IVF<nlist>,PQ<M>` in an id map) for gfx950.
//
// What it replaces: the reference's Faiss queryable as production configures it (ann_common.thrift:45: nprobe is "How many
// cells to visit in IVFPQ"; FaissIndexer.scala:82-92 hands any factory string to index_factory).  The contract is
// include/ivfpq_ann.h; the coarse half is that of ivf_ann.hip, whose kernels for it are shared through ivf_kernels.h.
//
// Shape of the computation.
//   * The coarse quantizer is a dann_index over the centroids, used through the prepared-search seam exactly as
//     ivf_ann.hip uses it.  ivfpq_index_train obtains the centroids from ivf_index_train, so the two index types train
//     the same cells from the same arguments.
//   * The rows are not kept.  An add prepares a slab of rows (fp16), assigns it, encodes it and keeps M code bytes, the id
//     and the cell per row, in the order added.  The lists are laid out again from that: every list starts on a block of
//     64 rows, a block is [M / 4][64] dwords -- lane r of a wave reads the four codes 4g .. 4g + 3 of row r with one
//     coalesced 256-byte load -- in (cell, id) order, beside the slot's rank in id order.
//   * encode_kernel: one workgroup per (64 rows, subspace).  The residuals r = fl32(x - centroid[cell]) of the tile go to
//     LDS, the subspace's codebook is staged through LDS 64 codewords at a time; wave w evaluates codewords 16w .. 16w+15
//     of the stage (the codeword is a broadcast LDS read), a lane owns a row.  Codebook training uses the same kernel
//     for its assignment step, and pq_mean_kernel (one workgroup per codeword, members compacted in position order,
//     summed in fp64 by one thread per component) for the means.
//   * adc_scan_kernel, the hot path: one workgroup per (query, probed cell) pair, the pairs sorted by cell so that
//     neighbouring workgroups read the same list from L2.  The workgroup builds the pair's table [M][256] in LDS
//     (thread j owns codeword j of every subspace), then its four waves stride over the list's blocks; a lane owns a
//     row and adds M table entries in ascending m, starting from 0 (L2) or <q, c> (InnerProduct / Cosine).  Survivors
//     go to the per-query buffer of ivf_ann.hip (CAP = 8192, one integer atomic per wave and block), with its arm / refine
//     rounds.
//   * Select sorts a query's survivors by (score desc, rank in id order asc), as ivf_ann.hip's select does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include "../../include/dense_ann.h"
#include "../../include/ivf_ann.h"
#include "../../include/ivfpq_ann.h"
#include "../../include/polysemous_ann.h"
#include "sann_device.h"  // mix64
#include "ivf_device_rows.h"
#include "faiss_restore.h"
#include "ivf_core.h"

namespace {

constexpr int KSUB = 256;    // codewords per sub-quantizer
constexpr int MAX_M = 64;
constexpr int LBLOCK = 64;   // rows per list block
constexpr int ENC_ROWS = 64; // rows per encoder workgroup
constexpr int ENC_STAGE = 64;  // codewords staged in LDS at a time

// ---------------------------------------------------------------------------------------------
// encoder: code[row][m] = argmin_j ||r_m - cb[m][j]||^2 in fp32, ties to the lower j.  grid (row tiles, M), 256 threads.
// The code of (row, m) is written at codes[row * row_stride + m * m_stride]: [n][M] for an add, [M][n] for training.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void encode_kernel(const _Float16 *__restrict__ flat, const int32_t *__restrict__ cell,
                                                     const float *__restrict__ cent, const float *__restrict__ cb, int64_t n,
                                                     int d, int dsub, uint8_t *__restrict__ codes, int64_t row_stride,
                                                     int64_t m_stride) {
  extern __shared__ float enc_lds[];
  float *s_r = enc_lds;                     // [dsub][ENC_ROWS]
  float *s_cb = enc_lds + dsub * ENC_ROWS;  // [ENC_STAGE][dsub]
  __shared__ float s_best[4][ENC_ROWS];
  __shared__ int s_arg[4][ENC_ROWS];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, m = blockIdx.y;
  const int64_t row0 = (int64_t)blockIdx.x * ENC_ROWS;
  for (int e = t; e < dsub * ENC_ROWS; e += 256) {
    const int r = e / dsub, i = e % dsub;
    const int64_t row = row0 + r;
    float v = 0.0f;
    if (row < n) v = (float)flat[(size_t)row * d + m * dsub + i] - cent[(size_t)cell[row] * d + m * dsub + i];
    s_r[i * ENC_ROWS + r] = v;
  }
  float best = INFINITY;
  int arg = 0;
  const float *cbm = cb + (size_t)m * KSUB * dsub;
  for (int j0 = 0; j0 < KSUB; j0 += ENC_STAGE) {
    __syncthreads();
    for (int e = t; e < ENC_STAGE * dsub; e += 256) s_cb[e] = cbm[(size_t)j0 * dsub + e];
    __syncthreads();
    for (int jj = 0; jj < 16; jj += 4) {
      const float *c0 = s_cb + (w * 16 + jj) * dsub;
      float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
      for (int i = 0; i < dsub; ++i) {
        const float r = s_r[i * ENC_ROWS + lane];
        const float e0 = r - c0[i], e1 = r - c0[dsub + i], e2 = r - c0[2 * dsub + i], e3 = r - c0[3 * dsub + i];
        a0 += e0 * e0;
        a1 += e1 * e1;
        a2 += e2 * e2;
        a3 += e3 * e3;
      }
      const int j = j0 + w * 16 + jj;
      if (a0 < best) { best = a0; arg = j; }
      if (a1 < best) { best = a1; arg = j + 1; }
      if (a2 < best) { best = a2; arg = j + 2; }
      if (a3 < best) { best = a3; arg = j + 3; }
    }
  }
  s_best[w][lane] = best;
  s_arg[w][lane] = arg;
  __syncthreads();
  if (w == 0 && row0 + lane < n) {
#pragma unroll
    for (int u = 1; u < 4; ++u) {
      const float b = s_best[u][lane];
      const int a = s_arg[u][lane];
      if (b < best || (b == best && a < arg)) {
        best = b;
        arg = a;
      }
    }
    codes[(row0 + lane) * row_stride + m * m_stride] = (uint8_t)arg;
  }
}

// ---------------------------------------------------------------------------------------------
// codebook training
// ---------------------------------------------------------------------------------------------
// the initial codewords: cb[m][j] = the m-th piece of the residual of training row picks[m][j]
__global__ void pq_pick_kernel(const _Float16 *__restrict__ flat, const int32_t *__restrict__ cell, const float *__restrict__ cent,
                               const int64_t *__restrict__ picks, int M, int d, int dsub, float *__restrict__ cb) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)M * KSUB * dsub) return;
  const int i = (int)(e % dsub), m = (int)(e / ((int64_t)KSUB * dsub));
  const int64_t row = picks[e / dsub];
  cb[e] = (float)flat[(size_t)row * d + m * dsub + i] - cent[(size_t)cell[row] * d + m * dsub + i];
}

// One workgroup per codeword (j, m): the rows that carry it are found 256 at a time and compacted in position order;
// component i of the mean is then summed by thread i over them, in fp64 -- a fixed order, no floating-point atomics.
// A codeword without members keeps its value.  codes are [M][n].
__global__ __launch_bounds__(256) void pq_mean_kernel(const _Float16 *__restrict__ flat, const int32_t *__restrict__ cell,
                                                      const float *__restrict__ cent, const uint8_t *__restrict__ codes, int64_t n,
                                                      int d, int dsub, float *__restrict__ cb) {
  __shared__ uint32_t s_rows[256];
  __shared__ uint32_t s_wcnt[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, j = blockIdx.x, m = blockIdx.y;
  const uint8_t *cm = codes + (size_t)m * n;
  double acc = 0.0;
  uint32_t members = 0;
  for (int64_t r0 = 0; r0 < n; r0 += 256) {
    const int64_t row = r0 + t;
    const bool mine = row < n && cm[row] == (uint8_t)j;
    const unsigned long long mask = __ballot(mine);
    if (lane == 0) s_wcnt[w] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t base = 0;
    for (int u = 0; u < w; ++u) base += s_wcnt[u];
    const uint32_t total = s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
    if (mine) s_rows[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t)row;
    __syncthreads();
    if (t < dsub)
      for (uint32_t u = 0; u < total; ++u) {
        const uint32_t rr = s_rows[u];
        const float r = (float)flat[(size_t)rr * d + m * dsub + t] - cent[(size_t)cell[rr] * d + m * dsub + t];
        acc += (double)r;
      }
    members += total;
    __syncthreads();
  }
  if (t < dsub && members > 0) cb[((size_t)m * KSUB + j) * dsub + t] = (float)(acc / (double)members);
}

// ---------------------------------------------------------------------------------------------
// list construction: the codes of row j of the (cell, id) order go to its list's next slot.  One thread per (row, 4 codes).
// ---------------------------------------------------------------------------------------------
__global__ void scatter_codes_kernel(const uint32_t *__restrict__ codes4 /*[n][M/4]*/, int64_t n, int M4,
                                     const uint32_t *__restrict__ cell_sorted, const uint32_t *__restrict__ ord,
                                     const uint32_t *__restrict__ perm, const uint32_t *__restrict__ start,
                                     const uint32_t *__restrict__ boff, uint32_t *__restrict__ lc, uint32_t *__restrict__ lrank) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * M4) return;
  const int64_t j = e / M4;
  const int g = (int)(e % M4);
  const uint32_t c = cell_sorted[j], rank = ord[j], src = perm[rank];
  const size_t slot = (size_t)boff[c] * LBLOCK + (size_t)(j - start[c]);
  const size_t blk = slot / LBLOCK;
  const int r = (int)(slot % LBLOCK);
  lc[(blk * M4 + g) * LBLOCK + r] = codes4[(size_t)src * M4 + g];
  if (g == 0) lrank[slot] = rank;
}
// one thread per cell: its share of the rows scanned (integers: any order gives the sum)
__global__ void rows_scanned_kernel(const uint32_t *__restrict__ per_cell, const uint32_t *__restrict__ sizes, int nlist,
                                    unsigned long long *__restrict__ rows_scanned) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nlist) return;
  const uint32_t cnt = per_cell[c];
  if (cnt) atomicAdd(rows_scanned, (unsigned long long)cnt * sizes[c]);
}

// ---------------------------------------------------------------------------------------------
// the ADC scan
// ---------------------------------------------------------------------------------------------
struct AdcArgs {
  const uint32_t *lc;       // list codes [block][M/4][64]
  const uint32_t *boff;     // first block of a cell's list
  const uint32_t *sizes;    // its rows
  const _Float16 *q16;      // prepared queries of the chunk, row-major [nq][d]
  const float *cent;        // centroids, fp32 [nlist][d]
  const float *cb;          // codebooks [M][256][dsub]
  const uint32_t *pair_cell, *pair_q;  // the pairs sorted by cell
  const float *tau;         // [nq]: emit scores >= tau; +inf = the query is finished
  uint32_t *cnt;            // [nq]
  Survivor *surv;           // [nq][CAP]
  int d, M, dsub, metric;
};

// what the Hamming-filtered scan (include/polysemous_ann.h) is given beside AdcArgs
struct HtArgs {
  const int32_t *probes;       // the chunk's rows of the probe export, [nq][nprobe]
  uint8_t *qcodes;             // the chunk's rows of the query-code export, [nq][nprobe][M]
  unsigned long long *scored;  // the rows that pass the filter are counted here in the first round, NULL in a later one
  int nprobe, ht;
};

// s_code[m] = argmin_j tab[m][j], ties to the lower j: wave w takes subspaces w, w + 4, ...; a lane looks at entries lane,
// lane + 64, ... in ascending order, then a fixed xor tree over (value, j)
__device__ __forceinline__ void query_code(const float *__restrict__ tab, int M, int lane, int w, uint8_t *__restrict__ s_code) {
  for (int m = w; m < M; m += 4) {
    const float *tb = tab + m * KSUB;
    float best = tb[lane];
    int arg = lane;
#pragma unroll
    for (int u = 1; u < 4; ++u) {
      const float v = tb[lane + 64 * u];
      if (v < best) {
        best = v;
        arg = lane + 64 * u;
      }
    }
    for (int o = 32; o; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oa = __shfl_xor(arg, o, 64);
      if (ov < best || (ov == best && oa < arg)) {
        best = ov;
        arg = oa;
      }
    }
    if (lane == 0) s_code[m] = (uint8_t)arg;
  }
}

// HT = false is ivfpq_search's scan, statement for statement what it was before the filter existed.  HT = true: the pair's
// query code (the encoding of fl32(q - centroid) by the encoder rule: for L2 an arg-min over the table, which holds exactly
// those distances; otherwise a pass over the codebook that borrows the table's LDS before the table is built) goes to M
// bytes of LDS behind s_u and to the export; a lane XORs its row's code dwords against it (a broadcast read) and only a
// row at Hamming distance < ht adds its table entries -- the same additions in the same order.
template <bool HT>
__device__ __forceinline__ void adc_scan_body(const AdcArgs &a, const HtArgs &h) {
  extern __shared__ float adc_lds[];
  float *s_tab = adc_lds;               // [M][256]
  float *s_u = adc_lds + a.M * KSUB;    // [d]: q - centroid (L2) or q
  __shared__ float s_qc;
  __shared__ int s_slot;  // HT: where the pair's cell stands in the query's row of probes (-1: nowhere)
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int d = a.d, M = a.M, dsub = a.dsub;
  const uint32_t cell = a.pair_cell[blockIdx.x], q = a.pair_q[blockIdx.x];
  const uint32_t size = a.sizes[cell];
  const float thr = a.tau[q];
  if constexpr (HT) {
    if (!(thr < INFINITY)) return;  // a fallback round this query is not part of (an empty list still has a query code)
  } else {
    if (size == 0 || !(thr < INFINITY)) return;  // an empty list, or a fallback round this query is not part of
  }
  const bool l2 = a.metric == IVF_METRIC_L2;
  const _Float16 *qp = a.q16 + (size_t)q * d;
  const float *cp = a.cent + (size_t)cell * d;
  uint8_t *s_code = (uint8_t *)(s_u + d);  // HT: [M], read back as M / 4 dwords
  if constexpr (HT) {
    if (t == 0) s_slot = -1;
    __syncthreads();
    for (int j = t; j < h.nprobe; j += 256)
      if ((uint32_t)h.probes[(size_t)q * h.nprobe + j] == cell) s_slot = j;
  }
  for (int i = t; i < d; i += 256) s_u[i] = l2 ? (float)qp[i] - cp[i] : (float)qp[i];
  if (w == 0) {
    // <q, c>: lane l sums the products of components l, l + 64, ... in ascending order, then a fixed shuffle tree
    float p = 0.0f;
    if (!l2)
      for (int i = lane; i < d; i += 64) p += (float)qp[i] * cp[i];
    for (int o = 32; o; o >>= 1) p += __shfl_xor(p, o, 64);
    if (lane == 0) s_qc = p;
  }
  __syncthreads();
  if constexpr (HT) {
    if (!l2) {
      // ||fl32(q - c)_m - cb[m][j]||^2 as the encoder sums it, thread j owning codeword j; the table's LDS holds them for now
      for (int m = 0; m < M; ++m) {
        const float *cw = a.cb + ((size_t)m * KSUB + t) * dsub;
        const float *u = s_u + m * dsub, *c = cp + m * dsub;
        float acc = 0.0f;
        for (int i = 0; i < dsub; ++i) {
          const float r = u[i] - c[i];
          const float e = r - cw[i];
          acc += e * e;
        }
        s_tab[m * KSUB + t] = acc;
      }
      __syncthreads();
      query_code(s_tab, M, lane, w, s_code);
      __syncthreads();
    }
  }
  // the table: thread j owns codeword j of every subspace, components in ascending order
  for (int m = 0; m < M; ++m) {
    const float *cw = a.cb + ((size_t)m * KSUB + t) * dsub;
    const float *u = s_u + m * dsub;
    float acc = 0.0f;
    if ((dsub & 3) == 0) {
      for (int i = 0; i < dsub; i += 4) {
        const float4 c4 = *(const float4 *)(cw + i);
        if (l2) {
          const float e0 = u[i] - c4.x, e1 = u[i + 1] - c4.y, e2 = u[i + 2] - c4.z, e3 = u[i + 3] - c4.w;
          acc += e0 * e0;
          acc += e1 * e1;
          acc += e2 * e2;
          acc += e3 * e3;
        } else {
          acc += u[i] * c4.x;
          acc += u[i + 1] * c4.y;
          acc += u[i + 2] * c4.z;
          acc += u[i + 3] * c4.w;
        }
      }
    } else {
      for (int i = 0; i < dsub; ++i) {
        if (l2) {
          const float e = u[i] - cw[i];
          acc += e * e;
        } else {
          acc += u[i] * cw[i];
        }
      }
    }
    s_tab[m * KSUB + t] = acc;
  }
  __syncthreads();
  if constexpr (HT) {
    if (l2) {
      query_code(s_tab, M, lane, w, s_code);
      __syncthreads();
    }
    if (t < M && s_slot >= 0) h.qcodes[((size_t)q * h.nprobe + s_slot) * M + t] = s_code[t];
  }
  const float acc0 = l2 ? 0.0f : s_qc;
  const int M4 = M >> 2;
  const uint32_t b0 = a.boff[cell], nb = (size + (uint32_t)LBLOCK - 1u) / (uint32_t)LBLOCK;
  unsigned long long scored = 0;  // HT: the wave's rows that passed the filter (the same in every lane)
  for (uint32_t blk = w; blk < nb; blk += 4) {
    const size_t gb = (size_t)b0 + blk;
    const uint32_t *cp4 = a.lc + gb * M4 * LBLOCK + lane;
    bool keep = true;
    if constexpr (HT) {
      const uint32_t *qc4 = (const uint32_t *)s_code;
      int ham = 0;
      for (int g = 0; g < M4; ++g) ham += __popc(cp4[(size_t)g * LBLOCK] ^ qc4[g]);
      keep = blk * (uint32_t)LBLOCK + (uint32_t)lane < size && ham < h.ht;
      scored += (unsigned long long)__popcll(__ballot(keep));
    }
    float acc = acc0;
    if (keep) {
      for (int g = 0; g < M4; ++g) {
        const uint32_t c4 = cp4[(size_t)g * LBLOCK];
        const float *tb = s_tab + (g * 4) * KSUB;
        acc += tb[c4 & 255u];
        acc += tb[KSUB + ((c4 >> 8) & 255u)];
        acc += tb[2 * KSUB + ((c4 >> 16) & 255u)];
        acc += tb[3 * KSUB + (c4 >> 24)];
      }
    }
    const float score = l2 ? -acc : acc;
    // the wave's survivors take consecutive slots, reserved by one integer atomic of its first surviving lane
    const bool pass = keep && blk * (uint32_t)LBLOCK + (uint32_t)lane < size && score >= thr;
    const unsigned long long mask = __ballot(pass);
    if (mask == 0) continue;
    const int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(&a.cnt[q], (uint32_t)__popcll(mask));
    base = __shfl(base, leader, 64);
    const uint32_t pos = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (pass && pos < (uint32_t)CAP) a.surv[(size_t)q * CAP + pos] = Survivor{score, (uint32_t)(gb * LBLOCK) + (uint32_t)lane};
  }
  if constexpr (HT) {
    if (h.scored && lane == 0 && scored) atomicAdd(h.scored, scored);  // one integer atomic per wave
  }
}

__global__ __launch_bounds__(256) void adc_scan_kernel(AdcArgs a) { adc_scan_body<false>(a, HtArgs{}); }
__global__ __launch_bounds__(256) void adc_scan_ht_kernel(AdcArgs a, HtArgs h) { adc_scan_body<true>(a, h); }

// per query: sort survivors by (score desc, rank in id order asc), emit the k nearest as distances (ivf_ann.hip's select
// with this index's scores: -s for L2, the similarity otherwise).  POSITIONS: emit instead, for the re-rank of
// refine_ann.hip, the k nearest as add-order positions perm[rank] (-1 past the count) beside their ranks.
template <bool POSITIONS>
__global__ __launch_bounds__(512) void pq_select_kernel(const Survivor *__restrict__ surv, const uint32_t *__restrict__ done_cnt,
                                                        const uint32_t *__restrict__ lrank, const int64_t *__restrict__ ids_sorted,
                                                        int metric, int k, float *__restrict__ out_dist,
                                                        int64_t *__restrict__ out_ids, int32_t *__restrict__ out_counts,
                                                        const uint32_t *__restrict__ perm, int32_t *__restrict__ out_pos,
                                                        uint32_t *__restrict__ out_rank) {
  extern __shared__ unsigned long long keys[];
  const int q = blockIdx.x;
  const uint32_t c = select_sorted(surv, done_cnt, lrank, q, keys);
  const uint32_t m = min(c, (uint32_t)k);
  if constexpr (POSITIONS) {
    for (uint32_t i = threadIdx.x; i < (uint32_t)k; i += blockDim.x) {
      int32_t pos = -1;
      uint32_t rank = 0;
      if (i < m) {
        rank = 0xffffffffu - (uint32_t)keys[i];
        pos = (int32_t)perm[rank];
      }
      out_pos[(size_t)q * k + i] = pos;
      out_rank[(size_t)q * k + i] = rank;
    }
  } else {
    for (uint32_t i = threadIdx.x; i < (uint32_t)k; i += blockDim.x) {
      float dist = 0.0f;
      int64_t id = 0;
      if (i < m) {
        unsigned long long key = keys[i];
        float sc = key2f((uint32_t)(key >> 32));
        id = ids_sorted[0xffffffffu - (uint32_t)key];
        if (metric == IVF_METRIC_L2) dist = sqrtf(fmaxf(0.0f, -sc));
        else dist = 1.0f - sc;
      }
      out_dist[(size_t)q * k + i] = dist;
      out_ids[(size_t)q * k + i] = id;
    }
  }
  if (threadIdx.x == 0) out_counts[q] = (int32_t)m;
}

// where the select step of a search writes when it serves ivfpq_internal::search_positions (device buffers)
struct PosOut {
  int32_t *pos;
  uint32_t *rank;
  int32_t *cnt;
};

}  // namespace

struct ivfpq_index : IvfBase {
  int M = 0, dsub = 0;
  Buf cent, cb;  // centroids fp32 [nlist][d] (the stored fp16 values), codebooks fp32 [M][256][dsub]
  // per row, in the order added
  Buf codes;
  // the lists' payload
  Buf lc;
  // per-call scratch: a slab of prepared rows, the prepared queries
  Buf flat, sumsq, q16;
  // polysemous_ann.h: the flag of the training, and the last search with ht > 0
  bool polysemous = false;
  Buf qcodes, scored_acc;
  int32_t qc_nq = 0, qc_nprobe = 0;
  int64_t last_scored = 0;
};

namespace {

int check_shape(int32_t metric, int32_t d, int32_t nlist, int32_t M) {
  if (int rc = check_shape(metric, d, nlist)) return rc;
  if (M < 4 || M > MAX_M || M % 4) return fail(IVF_EINVAL, "M must be a multiple of 4 in 4..64");
  if (d % M) return fail(IVF_EINVAL, "M must divide the dimension");
  return IVF_OK;
}

size_t encode_lds_bytes(int dsub) { return (size_t)(ENC_ROWS + ENC_STAGE) * dsub * sizeof(float); }
size_t adc_lds_bytes(int M, int d) { return ((size_t)M * KSUB + d) * sizeof(float); }
size_t adc_ht_lds_bytes(int M, int d) { return adc_lds_bytes(M, d) + (size_t)M; }  // + the query code

int new_index(int32_t device, int32_t metric, int32_t d, int32_t nlist, int32_t M, std::unique_ptr<ivfpq_index> &ix) {
  ITRY(hipSetDevice(device));
  ix.reset(new ivfpq_index);
  if (int rc = init_base(ix.get(), device, metric, d, nlist)) return rc;
  ix->M = M;
  ix->dsub = d / M;
  ITRY(ix->cent.reserve((size_t)nlist * d * sizeof(float)));
  ITRY(ix->cb.reserve((size_t)M * KSUB * ix->dsub * sizeof(float)));
  // both kernels size their LDS by the shape: up to 64 KiB (encoder, dsub = 128) and 66 KiB (scan, M = 64, d = 512)
  ITRY(hipFuncSetAttribute((const void *)encode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)encode_lds_bytes(MAX_D / 4)));
  ITRY(hipFuncSetAttribute((const void *)adc_scan_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)adc_lds_bytes(MAX_M, MAX_D)));
  ITRY(hipFuncSetAttribute((const void *)adc_scan_ht_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)adc_ht_lds_bytes(MAX_M, MAX_D)));
  ITRY(hipFuncSetAttribute((const void *)pq_select_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SELECT_LDS));
  ITRY(hipFuncSetAttribute((const void *)pq_select_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SELECT_LDS));
  return IVF_OK;
}

// the coarse quantizer over the given centroids (host, fp32 [nlist][d]); the index keeps the values it stores as fp32
int set_centroids(ivfpq_index *ix, const float *centroids) {
  const size_t bytes = (size_t)ix->nlist * ix->d * sizeof(float);
  ITRY(hipMemcpy(ix->cent.p, centroids, bytes, hipMemcpyHostToDevice));
  dann_index *c = nullptr;
  DCALL(ann_by_id::dann_build_device(ix->device, ix->metric, ix->nlist, ix->d, ix->cent.as<float>(), &c));
  if (ix->coarse) (void)dann_index_destroy(ix->coarse);
  ix->coarse = c;
  std::vector<float> stored((size_t)ix->nlist * ix->d);
  DCALL(dann_index_get_vectors(ix->coarse, 0, ix->nlist, stored.data()));
  ITRY(hipMemcpy(ix->cent.p, stored.data(), bytes, hipMemcpyHostToDevice));
  return IVF_OK;
}

int encode_rows(ivfpq_index *ix, const _Float16 *flat, const int32_t *cell, int64_t n, uint8_t *codes, int64_t row_stride,
                int64_t m_stride) {
  if (n == 0) return IVF_OK;
  hipLaunchKernelGGL(encode_kernel, dim3(blocks_for(n, ENC_ROWS), ix->M), dim3(256), encode_lds_bytes(ix->dsub), 0, flat, cell,
                     ix->cent.as<float>(), ix->cb.as<float>(), n, ix->d, ix->dsub, codes, row_stride, m_stride);
  ITRY(hipGetLastError());
  return IVF_OK;
}

using ivfpq_internal::slab_rows;

// all lists again from the codes in the order added: blocks of LBLOCK rows, [M / 4][LBLOCK] dwords each, beside the rank
int layout_lists(ivfpq_index *ix) {
  return layout_lists(ix, LBLOCK, [ix](size_t slots) -> int {
    const int M4 = ix->M >> 2;
    ITRY(ix->lc.reserve(slots * M4 * sizeof(uint32_t)));
    ITRY(hipMemset(ix->lc.p, 0, slots * M4 * sizeof(uint32_t)));
    hipLaunchKernelGGL(scatter_codes_kernel, dim3(blocks_for(ix->n * M4)), dim3(256), 0, 0, ix->codes.as<uint32_t>(), ix->n, M4,
                       ix->cell_sorted.as<uint32_t>(), ix->ord.as<uint32_t>(), ix->perm.as<uint32_t>(), ix->start.as<uint32_t>(),
                       ix->boff.as<uint32_t>(), ix->lc.as<uint32_t>(), ix->lrank.as<uint32_t>());
    ITRY(hipGetLastError());
    return IVF_OK;
  });
}

// the rows whose residuals are the initial codewords: picks[m][j], by the rule of ivfpq_ann.h
std::vector<int64_t> initial_picks(int M, int64_t n, uint64_t seed) {
  std::vector<int64_t> picks;
  picks.reserve((size_t)M * KSUB);
  for (int m = 0; m < M; ++m) {
    std::unordered_set<int64_t> seen;
    const uint64_t base = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(m + 1);
    for (uint64_t t = 0; (int)seen.size() < KSUB; ++t) {
      const int64_t r = (int64_t)(sann::mix64(base + t) % (uint64_t)n);
      if (seen.insert(r).second) picks.push_back(r);
    }
  }
  return picks;
}

// the M codebooks on the residuals of the n prepared training rows
int train_codebooks(ivfpq_index *ix, const _Float16 *tflat, const float *tsumsq, int64_t n, int rounds, uint64_t seed) {
  const int M = ix->M, d = ix->d, dsub = ix->dsub;
  Buf tcell, tcodes, picks_d;
  ITRY(tcell.reserve((size_t)n * 4));
  ITRY(tcodes.reserve((size_t)n * M));
  if (int rc = assign_rows(ix, tflat, tsumsq, n, tcell.as<int32_t>())) return rc;
  const std::vector<int64_t> picks = initial_picks(M, n, seed);
  ITRY(picks_d.reserve(picks.size() * 8));
  ITRY(hipMemcpy(picks_d.p, picks.data(), picks.size() * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(pq_pick_kernel, dim3(blocks_for((int64_t)M * KSUB * dsub)), dim3(256), 0, 0, tflat, tcell.as<int32_t>(),
                     ix->cent.as<float>(), picks_d.as<int64_t>(), M, d, dsub, ix->cb.as<float>());
  ITRY(hipGetLastError());
  for (int it = 0; it < rounds; ++it) {
    if (int rc = encode_rows(ix, tflat, tcell.as<int32_t>(), n, tcodes.as<uint8_t>(), 1, n)) return rc;
    hipLaunchKernelGGL(pq_mean_kernel, dim3(KSUB, M), dim3(256), 0, 0, tflat, tcell.as<int32_t>(), ix->cent.as<float>(),
                       tcodes.as<uint8_t>(), n, d, dsub, ix->cb.as<float>());
    ITRY(hipGetLastError());
  }
  ITRY(hipDeviceSynchronize());
  return IVF_OK;
}

// One chunk of a search.  out_on_device (without po): out_dist / out_ids / out_counts are device buffers, which the select
// launch writes itself; otherwise it writes the index's own and finish_chunk brings them to the host.
int search_chunk(ivfpq_index *ix, int32_t q0, int32_t nq, const float *queries, bool on_device, const int64_t *pos, int32_t k,
                 int32_t nprobe, float *out_dist, int64_t *out_ids, int32_t *out_counts, const PosOut *po, int32_t ht,
                 bool out_on_device) {
  const int d = ix->d, nlist = ix->nlist;
  hipStream_t st = 0;
  ITRY(ix->q16.reserve((size_t)nq * d * sizeof(_Float16)));
  if (int rc = probe_chunk(ix, q0, nq, queries, on_device, pos, k, nprobe, ix->q16.as<_Float16>(), nullptr)) return rc;
  // one workgroup per pair that names a cell: all nq * nprobe of them, but for an HNSW quantizer's short walks (ivf_core.h)
  const int64_t pairs = ix->chunk_pairs;
  hipLaunchKernelGGL(rows_scanned_kernel, dim3(blocks_for(nlist)), dim3(256), 0, st, ix->per_cell.as<uint32_t>(),
                     ix->sizes.as<uint32_t>(), nlist, ix->rows_acc.as<unsigned long long>());
  ITRY(hipGetLastError());

  // scan rounds
  AdcArgs a;
  a.lc = ix->lc.as<uint32_t>();
  a.boff = ix->boff.as<uint32_t>();
  a.sizes = ix->sizes.as<uint32_t>();
  a.q16 = ix->q16.as<_Float16>();
  a.cent = ix->cent.as<float>();
  a.cb = ix->cb.as<float>();
  a.pair_cell = ix->pair_cell_s.as<uint32_t>();
  a.pair_q = ix->pair_q_s.as<uint32_t>();
  a.tau = ix->tau.as<float>();
  a.cnt = ix->cnt.as<uint32_t>();
  a.surv = ix->surv.as<Survivor>();
  a.d = d;
  a.M = ix->M;
  a.dsub = ix->dsub;
  a.metric = ix->metric;
  HtArgs h{};
  if (ht > 0) {  // the Hamming-filtered scan of polysemous_ann.h (ix->qcodes and ix->scored_acc are the caller's)
    h.probes = ix->probes.as<int32_t>() + (size_t)q0 * nprobe;
    h.qcodes = ix->qcodes.as<uint8_t>() + (size_t)q0 * nprobe * ix->M;
    h.nprobe = nprobe;
    h.ht = ht;
  }
  int rounds = 0;
  if (int rc = scan_rounds(ix, nq, k, [&](int round, hipStream_t s) -> int {
        if (ht > 0) {
          h.scored = round == 0 ? ix->scored_acc.as<unsigned long long>() : nullptr;
          hipLaunchKernelGGL(adc_scan_ht_kernel, dim3((unsigned)pairs), dim3(256), adc_ht_lds_bytes(ix->M, d), s, a, h);
          ITRY(hipGetLastError());
        } else if (ix->n > 0) {
          hipLaunchKernelGGL(adc_scan_kernel, dim3((unsigned)pairs), dim3(256), adc_lds_bytes(ix->M, d), s, a);
          ITRY(hipGetLastError());
        }
        return IVF_OK;
      }, &rounds))
    return rc;

  if (po) {
    hipLaunchKernelGGL(pq_select_kernel<true>, dim3(nq), dim3(512), SELECT_LDS, st, ix->surv.as<Survivor>(),
                       ix->done_cnt.as<uint32_t>(), ix->lrank.as<uint32_t>(), ix->ids_sorted.as<int64_t>(), ix->metric, k,
                       (float *)nullptr, (int64_t *)nullptr, po->cnt + q0, ix->perm.as<uint32_t>(), po->pos + (size_t)q0 * k,
                       po->rank + (size_t)q0 * k);
  } else {
    hipLaunchKernelGGL(pq_select_kernel<false>, dim3(nq), dim3(512), SELECT_LDS, st, ix->surv.as<Survivor>(),
                       ix->done_cnt.as<uint32_t>(), ix->lrank.as<uint32_t>(), ix->ids_sorted.as<int64_t>(), ix->metric, k,
                       out_on_device ? out_dist : ix->o_dist.as<float>(), out_on_device ? out_ids : ix->o_ids.as<int64_t>(),
                       out_on_device ? out_counts : ix->o_cnt.as<int32_t>(), (const uint32_t *)nullptr, (int32_t *)nullptr,
                       (uint32_t *)nullptr);
  }
  ITRY(hipGetLastError());
  return finish_chunk(ix, nq, k, rounds, po || out_on_device ? nullptr : out_dist, out_ids, out_counts);
}

// ivfpq_index_train, over host rows or over rows that are on the device
int train_rows(int32_t device, int32_t metric, int32_t d, int32_t nlist, int32_t M, int64_t n_train, const float *train_vectors,
               bool on_device, int32_t niter, uint64_t seed, ivfpq_index_t **out) {
  if (!train_vectors || !out) return fail(IVF_EINVAL, "null argument");
  if (int rc = check_shape(metric, d, nlist, M)) return rc;
  if (n_train < std::max<int64_t>(nlist, KSUB)) return fail(IVF_EINVAL, "n_train must be at least max(nlist, 256)");
  if (n_train >= ((int64_t)1 << 31)) return fail(IVF_EINVAL, "n_train out of range");
  if (niter < -1) return fail(IVF_EINVAL, "niter must be -1 (initial picks), 0 (20 rounds) or a number of rounds");
  const int rounds = niter == 0 ? 20 : niter == -1 ? 0 : niter;
  // the coarse quantizer, trained as an IVF-Flat index trains it
  std::vector<float> centroids((size_t)nlist * d);
  {
    ivf_index_t *flat = nullptr;
    if (int rc = on_device ? ivf_internal::train_device(device, metric, d, nlist, n_train, train_vectors, niter, seed, &flat)
                           : ivf_index_train(device, metric, d, nlist, n_train, train_vectors, niter, seed, &flat))
      return fail(rc, std::string("coarse training: ") + ivf_last_error());
    const int rc = ivf_index_get_centroids(flat, centroids.data());
    const std::string msg = rc ? ivf_last_error() : "";
    (void)ivf_index_destroy(flat);
    if (rc) return fail(rc, "coarse training: " + msg);
  }
  std::unique_ptr<ivfpq_index> ix;
  if (int rc = new_index(device, metric, d, nlist, M, ix)) return rc;
  if (int rc = set_centroids(ix.get(), centroids.data())) return rc;
  // the training rows, prepared as stored rows are; they go with this call
  Buf tflat, tsumsq;
  ITRY(tflat.reserve((size_t)n_train * d * sizeof(_Float16)));
  ITRY(tsumsq.reserve((size_t)n_train * sizeof(float)));
  if (int rc = upload_rows(ix.get(), train_vectors, on_device, n_train, tflat.as<_Float16>(), tsumsq.as<float>())) return rc;
  if (int rc = train_codebooks(ix.get(), tflat.as<_Float16>(), tsumsq.as<float>(), n_train, rounds, seed)) return rc;
  *out = ix.release();
  return IVF_OK;
}

// new[m][perm[m][j]] = old[m][j].  One thread per component.
__global__ void renumber_codebooks_kernel(const float *__restrict__ old_cb, const uint8_t *__restrict__ perm, int M, int dsub,
                                          float *__restrict__ new_cb) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)M * KSUB * dsub) return;
  const int i = (int)(e % dsub), j = (int)((e / dsub) % KSUB), m = (int)(e / ((int64_t)KSUB * dsub));
  new_cb[((size_t)m * KSUB + perm[m * KSUB + j]) * dsub + i] = old_cb[e];
}

// the polysemous step of a training (polysemous_ann.h): one renumbering per subspace on at most 16 host threads, which
// share nothing but the read-only codebooks; then the codebooks are renumbered on the device.  The index holds no rows.
int make_polysemous(ivfpq_index *ix, uint64_t seed, int64_t anneal_iters) {
  const int M = ix->M, dsub = ix->dsub;
  const size_t count = (size_t)M * KSUB * dsub;
  std::vector<float> cb(count);
  ITRY(hipSetDevice(ix->device));
  ITRY(hipMemcpy(cb.data(), ix->cb.p, count * sizeof(float), hipMemcpyDeviceToHost));
  std::vector<uint8_t> perm((size_t)M * KSUB);
  std::vector<int> status((size_t)M, IVF_OK);
  std::vector<std::string> message((size_t)M);
  const int threads = std::min(M, 16);
  auto work = [&](int first) {
    for (int m = first; m < M; m += threads) {
      double before = 0, after = 0;
      status[(size_t)m] = polysemous_optimize_codebook(dsub, cb.data() + (size_t)m * KSUB * dsub, anneal_iters,
                                                       sann::mix64(seed + 0x9E3779B97F4A7C15ull * (uint64_t)(m + 1)),
                                                       perm.data() + (size_t)m * KSUB, &before, &after);
      if (status[(size_t)m]) message[(size_t)m] = polysemous_last_error();  // (thread-local: read where it was written)
    }
  };
  std::vector<std::thread> pool;
  for (int u = 1; u < threads; ++u) pool.emplace_back(work, u);
  work(0);
  for (auto &th : pool) th.join();
  for (int m = 0; m < M; ++m)
    if (status[(size_t)m]) return fail(status[(size_t)m], "polysemous training, subspace " + std::to_string(m) + ": " + message[(size_t)m]);
  Buf old_cb, perm_d;
  ITRY(old_cb.reserve(count * sizeof(float)));
  ITRY(perm_d.reserve(perm.size()));
  ITRY(hipMemcpy(old_cb.p, ix->cb.p, count * sizeof(float), hipMemcpyDeviceToDevice));
  ITRY(hipMemcpy(perm_d.p, perm.data(), perm.size(), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(renumber_codebooks_kernel, dim3(blocks_for((int64_t)count)), dim3(256), 0, 0, old_cb.as<float>(),
                     perm_d.as<uint8_t>(), M, dsub, ix->cb.as<float>());
  ITRY(hipGetLastError());
  ITRY(hipDeviceSynchronize());
  ix->polysemous = true;
  return IVF_OK;
}

// train_rows, then the polysemous step
int train_rows_polysemous(int32_t device, int32_t metric, int32_t d, int32_t nlist, int32_t M, int64_t n_train,
                          const float *train_vectors, bool on_device, int32_t niter, uint64_t seed, int64_t anneal_iters,
                          ivfpq_index_t **out) {
  if (anneal_iters < 0) return fail(IVF_EINVAL, "anneal_iters must be 0 (500000 steps) or a number of steps");
  if (!out) return fail(IVF_EINVAL, "null argument");
  ivfpq_index_t *ix = nullptr;
  if (int rc = train_rows(device, metric, d, nlist, M, n_train, train_vectors, on_device, niter, seed, &ix)) return rc;
  std::unique_ptr<ivfpq_index> hold(ix);
  if (int rc = make_polysemous(ix, seed, anneal_iters)) return rc;
  *out = hold.release();
  return IVF_OK;
}

// ivfpq_search, over host queries or over queries that are on the device; out_on_device: the three outputs are device buffers;
// pos != NULL: the device queries are the rows pos[0 .. nq) of the store whose first row is `queries` (probe_chunk), a
// chunk's positions at pos + q0
int search_rows(ivfpq_index_t *ix, int32_t nq, const float *queries, bool on_device, int32_t k, int32_t nprobe, float *out_dist,
                int64_t *out_ids, int32_t *out_counts, const PosOut *po = nullptr, int32_t ht = 0, bool out_on_device = false,
                const int64_t *pos = nullptr) {
  if (!ix || !queries) return fail(IVF_EINVAL, "null argument");
  if (po ? !po->pos || !po->rank || !po->cnt : !out_dist || !out_ids || !out_counts) return fail(IVF_EINVAL, "null argument");
  if (int rc = search_begin(ix, nq, k, &nprobe)) return rc;
  if (ht > 0) {
    ix->qc_nq = 0;  // (a failure below leaves no query codes to ask for)
    ITRY(ix->qcodes.reserve((size_t)nq * nprobe * ix->M));
    ITRY(ix->scored_acc.reserve(8));
    ITRY(hipMemset(ix->qcodes.p, 0, (size_t)nq * nprobe * ix->M));
    ITRY(hipMemset(ix->scored_acc.p, 0, 8));
  }
  if (int rc = search_chunks(ix, nq, [&](int32_t q0, int32_t m) -> int {
        return search_chunk(ix, q0, m, pos ? queries : queries + (size_t)q0 * ix->d, on_device, pos ? pos + q0 : nullptr, k, nprobe,
                            po ? nullptr : out_dist + (size_t)q0 * k,
                            po ? nullptr : out_ids + (size_t)q0 * k, po ? nullptr : out_counts + q0, po, ht, out_on_device);
      }))
    return rc;
  if (ht > 0) {
    unsigned long long scored = 0;
    ITRY(hipMemcpy(&scored, ix->scored_acc.p, 8, hipMemcpyDeviceToHost));
    ix->last_ctl += 8;
    ix->last_scored = (int64_t)scored;
    ix->qc_nq = nq;
    ix->qc_nprobe = nprobe;
  }
  return IVF_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// the device-rows seam (ivf_device_rows.h)
// ---------------------------------------------------------------------------------------------
int64_t ivfpq_internal::slab_rows(int d) { return stage_slab_rows(d); }

ivf_hq::State *ivfpq_internal::hnsw_quantizer(ivfpq_index *ix) { return hq_state(ix); }  // ivf_hnsw_quantizer_internal.h

int ivfpq_internal::train_device(int32_t device, int32_t metric, int32_t d, int32_t nlist, int32_t M, int64_t n_train,
                                 const float *d_rows, int32_t niter, uint64_t seed, ivfpq_index **out) try {
  return train_rows(device, metric, d, nlist, M, n_train, d_rows, true, niter, seed, out);
} ABI_CATCH

int ivfpq_internal::add_begin(ivfpq_index *ix, int64_t n, bool with_ids) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (n < 1) return fail(IVF_EINVAL, "n must be positive");
  if (int rc = check_ids_rule(ix, with_ids)) return rc;
  if (int rc = grow_rows(ix, n)) return rc;
  const int64_t n_old = ix->n, total = n_old + n;
  const int d = ix->d, M = ix->M;
  ITRY(ix->codes.grow_keep((size_t)n_old * M, (size_t)total * M));
  // a slab of rows at a time: prepare, assign, encode; the fp16 rows are scratch
  const int64_t slab = slab_rows(d);
  ITRY(ix->flat.reserve((size_t)std::min(slab, n) * d * sizeof(_Float16)));
  ITRY(ix->sumsq.reserve((size_t)std::min(slab, n) * sizeof(float)));
  return IVF_OK;
} ABI_CATCH

int ivfpq_internal::add_slab(ivfpq_index *ix, int64_t r0, int64_t m, const float *d_rows) try {
  const int64_t at = ix->n + r0;
  const int M = ix->M;
  if (int rc = prepare_slab(ix, d_rows, m, ix->flat.as<_Float16>(), ix->sumsq.as<float>())) return rc;
  int32_t *cell = ix->cell.as<int32_t>() + at;
  if (int rc = assign_rows(ix, ix->flat.as<_Float16>(), ix->sumsq.as<float>(), m, cell)) return rc;
  if (int rc = encode_rows(ix, ix->flat.as<_Float16>(), cell, m, ix->codes.as<uint8_t>() + (size_t)at * M, M, 1)) return rc;
  ITRY(hipDeviceSynchronize());
  return IVF_OK;
} ABI_CATCH

int ivfpq_internal::add_end(ivfpq_index *ix, int64_t n, const int64_t *ids) try {
  if (int rc = commit_add(ix, n, ids)) return rc;
  return layout_lists(ix);
} ABI_CATCH

int ivfpq_internal::search_device(ivfpq_index *ix, int32_t nq, const float *d_queries, int32_t k, int32_t nprobe, float *out_dist,
                                  int64_t *out_ids, int32_t *out_counts) try {
  return search_rows(ix, nq, d_queries, true, k, nprobe, out_dist, out_ids, out_counts);
} ABI_CATCH

int ivfpq_internal::search_positions(ivfpq_index *ix, int32_t nq, const float *d_queries, int32_t k, int32_t nprobe, int32_t *d_pos,
                                     uint32_t *d_rank, int32_t *d_counts) try {
  const PosOut po{d_pos, d_rank, d_counts};
  return search_rows(ix, nq, d_queries, true, k, nprobe, nullptr, nullptr, nullptr, &po);
} ABI_CATCH

int ivfpq_internal::train_device_polysemous(int32_t device, int32_t metric, int32_t d, int32_t nlist, int32_t M, int64_t n_train,
                                            const float *d_rows, int32_t niter, uint64_t seed, int64_t anneal_iters,
                                            ivfpq_index **out) try {
  return train_rows_polysemous(device, metric, d, nlist, M, n_train, d_rows, true, niter, seed, anneal_iters, out);
} ABI_CATCH

int ivfpq_internal::search_device_ht(ivfpq_index *ix, int32_t nq, const float *d_queries, int32_t k, int32_t nprobe, int32_t ht,
                                     float *out_dist, int64_t *out_ids, int32_t *out_counts) try {
  if (int rc = search_rows(ix, nq, d_queries, true, k, nprobe, out_dist, out_ids, out_counts, nullptr, std::max(ht, 0))) return rc;
  if (ht <= 0) ix->last_scored = ix->last_rows;
  return IVF_OK;
} ABI_CATCH

int ivfpq_internal::search_device_out(ivfpq_index *ix, int32_t nq, const float *d_queries, int32_t k, int32_t nprobe, int32_t ht,
                                      float *d_dist, int64_t *d_ids, int32_t *d_counts) try {
  if (int rc = search_rows(ix, nq, d_queries, true, k, nprobe, d_dist, d_ids, d_counts, nullptr, std::max(ht, 0), true)) return rc;
  if (ht <= 0) ix->last_scored = ix->last_rows;
  return IVF_OK;
} ABI_CATCH

int ivfpq_internal::search_store_out(ivfpq_index *ix, int32_t nq, const float *d_store_rows, const int64_t *d_pos, int32_t k,
                                     int32_t nprobe, int32_t ht, float *d_dist, int64_t *d_ids, int32_t *d_counts) try {
  if (!d_pos) return fail(IVF_EINVAL, "null argument");
  if (int rc = search_rows(ix, nq, d_store_rows, true, k, nprobe, d_dist, d_ids, d_counts, nullptr, std::max(ht, 0), true, d_pos))
    return rc;
  if (ht <= 0) ix->last_scored = ix->last_rows;
  return IVF_OK;
} ABI_CATCH

int64_t ivfpq_internal::last_control_bytes(const ivfpq_index *ix) { return ix->last_ctl; }
int64_t ivfpq_internal::last_control_upload_bytes(const ivfpq_index *ix) { return ix->last_ctl_up; }
std::shared_ptr<void> &ivfpq_internal::by_id_scratch(ivfpq_index *ix) { return ix->by_id; }

int ivfpq_internal::search_stats_unfiltered(ivfpq_index *ix) {
  if (!ix) return fail(IVF_EINVAL, "null index");
  ix->last_scored = ix->last_rows;
  return IVF_OK;
}

const int64_t *ivfpq_internal::device_ids_sorted(const ivfpq_index *ix) { return ix->ids_sorted.as<int64_t>(); }
int ivfpq_internal::device_of(const ivfpq_index *ix) { return ix->device; }

int ivfpq_internal::pq_train_plain(int32_t device, const _Float16 *d_rows16, int64_t n, int32_t d, int32_t M, bool init,
                                   int32_t rounds, uint64_t seed, float *d_cb, uint8_t *d_codes) try {
  if (!d_rows16 || !d_cb || !d_codes) return fail(IVF_EINVAL, "null argument");
  if (n < KSUB || n >= ((int64_t)1 << 31)) return fail(IVF_EINVAL, "a product quantiser needs 256 .. 2^31 - 1 rows");
  ITRY(hipSetDevice(device));
  const int dsub = d / M;
  Buf cell0, cent0, tcodes, picks_d;
  ITRY(cell0.reserve((size_t)n * 4));
  ITRY(cent0.reserve((size_t)d * sizeof(float)));
  ITRY(tcodes.reserve((size_t)n * M));
  ITRY(hipMemset(cell0.p, 0, (size_t)n * 4));
  ITRY(hipMemset(cent0.p, 0, (size_t)d * sizeof(float)));
  ITRY(hipFuncSetAttribute((const void *)encode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)encode_lds_bytes(MAX_D / 4)));
  if (init) {
    const std::vector<int64_t> picks = initial_picks(M, n, seed);
    ITRY(picks_d.reserve(picks.size() * 8));
    ITRY(hipMemcpy(picks_d.p, picks.data(), picks.size() * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(pq_pick_kernel, dim3(blocks_for((int64_t)M * KSUB * dsub)), dim3(256), 0, 0, d_rows16, cell0.as<int32_t>(),
                       cent0.as<float>(), picks_d.as<int64_t>(), M, d, dsub, d_cb);
    ITRY(hipGetLastError());
  }
  for (int it = 0; it <= rounds; ++it) {
    const bool last = it == rounds;  // the final encoding, [n][M]
    hipLaunchKernelGGL(encode_kernel, dim3(blocks_for(n, ENC_ROWS), M), dim3(256), encode_lds_bytes(dsub), 0, d_rows16,
                       cell0.as<int32_t>(), cent0.as<float>(), d_cb, n, d, dsub, last ? d_codes : tcodes.as<uint8_t>(),
                       last ? (int64_t)M : (int64_t)1, last ? (int64_t)1 : n);
    ITRY(hipGetLastError());
    if (last) break;
    hipLaunchKernelGGL(pq_mean_kernel, dim3(KSUB, M), dim3(256), 0, 0, d_rows16, cell0.as<int32_t>(), cent0.as<float>(),
                       tcodes.as<uint8_t>(), n, d, dsub, d_cb);
    ITRY(hipGetLastError());
  }
  ITRY(hipDeviceSynchronize());
  return IVF_OK;
} ABI_CATCH

// ---------------------------------------------------------------------------------------------
// restoring a saved index (faiss_restore.h)
// ---------------------------------------------------------------------------------------------
int64_t ivfpq_internal::restore_slab_rows(int32_t M) { return std::max<int64_t>(1, (int64_t)(32 << 20) / (M + 12)); }

int ivfpq_internal::restore_begin(int32_t device, int32_t metric, int32_t d, int32_t nlist, int32_t M, const float *centroids,
                                  const float *codebooks, int32_t ids_mode, int64_t n, ivfpq_index **out) try {
  if (!centroids || !codebooks || !out) return fail(IVF_EINVAL, "null argument");
  if (int rc = check_shape(metric, d, nlist, M)) return rc;
  if (int rc = check_restore(ids_mode, n)) return rc;
  std::unique_ptr<ivfpq_index> ix;
  if (int rc = new_index(device, metric, d, nlist, M, ix)) return rc;
  // the stored centroids are what the index keeps and what its coarse quantizer holds: neither is rounded or normalised again
  ITRY(hipMemcpy(ix->cent.p, centroids, (size_t)nlist * d * sizeof(float), hipMemcpyHostToDevice));
  DCALL(ann_by_id::dann_build_device(device, metric, nlist, d, ix->cent.as<float>(), &ix->coarse, true));
  ITRY(hipMemcpy(ix->cb.p, codebooks, (size_t)M * KSUB * ix->dsub * sizeof(float), hipMemcpyHostToDevice));
  ITRY(ix->codes.reserve((size_t)n * M));
  if (int rc = restore_open(ix.get(), ids_mode, n)) return rc;
  *out = ix.release();
  return IVF_OK;
} ABI_CATCH

int ivfpq_internal::restore_stage(ivfpq_index *ix, int64_t m, int64_t **ids, int32_t **cells, uint8_t **codes) try {
  return restore_staging(ix, m, ix ? restore_slab_rows(ix->M) : 0, ix ? (size_t)ix->M : 0, ids, cells, (void **)codes);
} ABI_CATCH

int ivfpq_internal::restore_slab(ivfpq_index *ix, int64_t r0, int64_t m) try {
  if (int rc = restore_rows(ix, r0, m, ix ? ix->codes.p : nullptr)) return rc;
  ix->rs.done = r0 + m;
  return IVF_OK;
} ABI_CATCH

int ivfpq_internal::restore_end(ivfpq_index *ix) try {
  if (int rc = restore_close(ix)) return rc;
  return ix->n > 0 ? layout_lists(ix) : IVF_OK;
} ABI_CATCH

int ivfpq_internal::export_rows(const ivfpq_index *ix, int64_t r0, int64_t m, int64_t *ids, int32_t *cells, uint8_t *codes) try {
  return export_columns(ix, r0, m, ids, cells, codes, ix ? ix->codes.p : nullptr, ix ? (size_t)ix->M : 0);
} ABI_CATCH

int ivfpq_internal::ids_mode(const ivfpq_index *ix) { return ix->ids_mode; }

extern "C" {

const char *ivfpq_last_error(void) { return g_err.c_str(); }

int ivfpq_index_load(int32_t device, int32_t metric, int32_t d, int32_t nlist, int32_t M, const float *centroids,
                     const float *codebooks, ivfpq_index_t **out) try {
  if (!centroids || !codebooks || !out) return fail(IVF_EINVAL, "null argument");
  if (int rc = check_shape(metric, d, nlist, M)) return rc;
  std::unique_ptr<ivfpq_index> ix;
  if (int rc = new_index(device, metric, d, nlist, M, ix)) return rc;
  if (int rc = set_centroids(ix.get(), centroids)) return rc;
  ITRY(hipMemcpy(ix->cb.p, codebooks, (size_t)M * KSUB * ix->dsub * sizeof(float), hipMemcpyHostToDevice));
  *out = ix.release();
  return IVF_OK;
} ABI_CATCH

int ivfpq_index_train(int32_t device, int32_t metric, int32_t d, int32_t nlist, int32_t M, int64_t n_train,
                      const float *train_vectors, int32_t niter, uint64_t seed, ivfpq_index_t **out) try {
  return train_rows(device, metric, d, nlist, M, n_train, train_vectors, false, niter, seed, out);
} ABI_CATCH

int ivfpq_index_add(ivfpq_index_t *ix, int64_t n, const float *vectors, const int64_t *ids) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (n < 0) return fail(IVF_EINVAL, "n must not be negative");
  if (int rc = check_ids_rule(ix, ids != nullptr)) return rc;
  if (n == 0) return IVF_OK;
  if (!vectors) return fail(IVF_EINVAL, "null vectors");
  if (int rc = ivfpq_internal::add_begin(ix, n, ids != nullptr)) return rc;
  const int64_t slab = slab_rows(ix->d);
  for (int64_t r0 = 0; r0 < n; r0 += slab) {
    const int64_t m = std::min(slab, n - r0);
    if (int rc = stage_rows(ix, vectors + r0 * ix->d, m)) return rc;
    if (int rc = ivfpq_internal::add_slab(ix, r0, m, ix->stage.as<float>())) return rc;
  }
  return ivfpq_internal::add_end(ix, n, ids);
} ABI_CATCH

int ivfpq_search(ivfpq_index_t *ix, int32_t nq, const float *queries, int32_t k, int32_t nprobe, float *out_dist,
                 int64_t *out_ids, int32_t *out_counts) try {
  return search_rows(ix, nq, queries, false, k, nprobe, out_dist, out_ids, out_counts);
} ABI_CATCH

int ivfpq_index_train_polysemous(int32_t device, int32_t metric, int32_t d, int32_t nlist, int32_t M, int64_t n_train,
                                 const float *train_vectors, int32_t niter, uint64_t seed, int64_t anneal_iters,
                                 ivfpq_index_t **out) try {
  return train_rows_polysemous(device, metric, d, nlist, M, n_train, train_vectors, false, niter, seed, anneal_iters, out);
} ABI_CATCH

int ivfpq_index_is_polysemous(const ivfpq_index_t *ix, int32_t *out) try {
  if (!ix || !out) return fail(IVF_EINVAL, "null argument");
  *out = ix->polysemous ? 1 : 0;
  return IVF_OK;
} ABI_CATCH

int ivfpq_search_ht(ivfpq_index_t *ix, int32_t nq, const float *queries, int32_t k, int32_t nprobe, int32_t ht, float *out_dist,
                    int64_t *out_ids, int32_t *out_counts) try {
  if (ht <= 0) {  // the filter is off: ivfpq_search itself
    if (int rc = ivfpq_search(ix, nq, queries, k, nprobe, out_dist, out_ids, out_counts)) return rc;
    ix->last_scored = ix->last_rows;
    return IVF_OK;
  }
  return search_rows(ix, nq, queries, false, k, nprobe, out_dist, out_ids, out_counts, nullptr, ht);
} ABI_CATCH

int ivfpq_last_query_codes(const ivfpq_index_t *ix, int32_t *nq, int32_t *nprobe, uint8_t *out) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (ix->qc_nq == 0) return fail(IVF_EINVAL, "no search with ht > 0 has run on this index: there are no query codes");
  if (nq) *nq = ix->qc_nq;
  if (nprobe) *nprobe = ix->qc_nprobe;
  if (out) {
    ITRY(hipSetDevice(ix->device));
    ITRY(hipMemcpy(out, ix->qcodes.p, (size_t)ix->qc_nq * ix->qc_nprobe * ix->M, hipMemcpyDeviceToHost));
  }
  return IVF_OK;
} ABI_CATCH

int ivfpq_last_ht_stats(const ivfpq_index_t *ix, int64_t *rows_scored) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (rows_scored) *rows_scored = ix->last_scored;
  return IVF_OK;
} ABI_CATCH

int ivfpq_index_info(const ivfpq_index_t *ix, int64_t *n, int32_t *d, int32_t *metric, int32_t *nlist, int32_t *M) try {
  if (int rc = index_info(ix, n, d, metric, nlist)) return rc;
  if (M) *M = ix->M;
  return IVF_OK;
} ABI_CATCH

int ivfpq_index_get_centroids(const ivfpq_index_t *ix, float *out) try { return get_centroids(ix, out); } ABI_CATCH

int ivfpq_index_get_codebooks(const ivfpq_index_t *ix, float *out) try {
  if (!ix || !out) return fail(IVF_EINVAL, "null argument");
  ITRY(hipSetDevice(ix->device));
  ITRY(hipMemcpy(out, ix->cb.p, (size_t)ix->M * KSUB * ix->dsub * sizeof(float), hipMemcpyDeviceToHost));
  return IVF_OK;
} ABI_CATCH

int ivfpq_index_get_codes(const ivfpq_index_t *ix, uint8_t *out) try {
  if (!ix || !out) return fail(IVF_EINVAL, "null argument");
  if (ix->n == 0) return IVF_OK;
  ITRY(hipSetDevice(ix->device));
  ITRY(hipMemcpy(out, ix->codes.p, (size_t)ix->n * ix->M, hipMemcpyDeviceToHost));
  return IVF_OK;
} ABI_CATCH

int ivfpq_index_list_sizes(const ivfpq_index_t *ix, int64_t *out) try { return list_sizes(ix, out); } ABI_CATCH

int ivfpq_index_get_assignment(const ivfpq_index_t *ix, int64_t *out_ids, int32_t *out_cells) try {
  return get_assignment(ix, out_ids, out_cells);
} ABI_CATCH

int ivfpq_last_probes(const ivfpq_index_t *ix, int32_t *nq, int32_t *nprobe, int32_t *out_cells) try {
  return last_probes(ix, nq, nprobe, out_cells);
} ABI_CATCH

int ivfpq_last_stats(const ivfpq_index_t *ix, int64_t *rows_scanned, int32_t *rounds, float *coarse_ms, float *scan_ms,
                     float *select_ms) try {
  return last_stats(ix, rows_scanned, rounds, coarse_ms, scan_ms, select_ms);
} ABI_CATCH

int ivfpq_index_destroy(ivfpq_index_t *ix) try {
  delete ix;
  return IVF_OK;
} ABI_CATCH

}  // extern "C"
