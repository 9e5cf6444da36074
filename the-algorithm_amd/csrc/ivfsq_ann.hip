// ivfsq_ann.hip -- inverted-file index with 8-bit scalar-quantised lists (`IVF<nlist>,SQ8` in an id map) on the gfx950
// matrix cores.
//
// What it serves: the factory strings the reference hands to Faiss (ann/src/main/scala/com/twitter/ann/faiss/
// FaissIndexer.scala:82-92: index_factory -> train -> add_with_ids), for the scalar quantiser QT_8bit over inverted lists;
// the semantics are fixed in include/ivfsq_ann.h.  The coarse quantizer, the list bookkeeping, the probe inversion, the
// survivor buffer with its fallback rounds and the select step are the shared core's (ivf_core.h, ivf_kernels.h,
// ivf_flat_lists.h, survivor_topk.h): this source adds the ranges, the encoder, the payload scatter, the query scaling and
// the scan.
//
// Shape of the computation.
//   * Ranges: per component the minimum and maximum of the prepared training rows, by integer atomicMin / atomicMax on the
//     order-preserving key of survivor_topk.h's f2key -- exact, whatever the order.  step = vdiff / 255 is one fp32 division
//     on the host; vmin and step live on the device as fp32 [d].
//   * An add prepares a slab of rows as fp16 (the core's store_rows_kernel), assigns it, and encodes it: one wave per row,
//     a byte per component and |xhat|^2 in fp64.  The fp16 rows go with the slab.
//   * The rows are kept twice, as codes: row-major uint8 [n][d] in the order added (what an add re-lays the lists out from,
//     and what ivfsq_index_get_codes exports), and in the lists -- one contiguous buffer in which every list starts on a
//     32-row block, in (cell, id) order, beside a per-slot bias (0, -|xhat|^2/2 for L2, -inf for the padding of a list's
//     last block) and the slot's rank in id order.
//   * A block of 32 rows is 32 d bytes in the A-fragment order of v_mfma_f32_32x32x16_f16: lane (r, h) = h * 32 + r owns
//     components 16 s + 8 h .. + 8 of row r in k-step s (S = d / 16 k-steps), 8 contiguous bytes.  Two k-steps are paired
//     into one 16-byte load:
//         [block][pair p < S / 2][lane 0..63][k-step 2p: 8 bytes | k-step 2p + 1: 8 bytes]      1 KiB per pair
//         [block][the last k-step, if S is odd][lane 0..63][8 bytes]                            512 B
//     so a wave's load is one contiguous, coalesced 1-KiB (or 512-B) run: half the bytes the flat scan reads per MFMA.
//     No LDS staging of list bytes.
//   * A search: the core's probe_chunk (fp16 queries, coarse search, pairs sorted by cell), then the query kernel turns
//     the chunk's fp16 rows into s = fp16(q * step) in B-fragment order and into b_q, then the scan: one workgroup per
//     Group (a cell and <= 32 of the queries that probe it), the group's s fragments gathered once into LDS, the four waves
//     stride over the cell's blocks, the accumulator starts from the bias, per k-step the 8 code bytes of a lane are
//     widened to fp16 exactly (v_perm_b32 puts each byte under 0x64: the half 1024 + b; a packed subtract of 1024 leaves b)
//     and go to the MFMA, b_q of the lane's query is added, and the threshold test, the survivor atomics, the fallback
//     rounds and the select step are the flat index's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dense_ann.h"
#include "../../include/ivf_ann.h"
#include "../../include/ivfsq_ann.h"
#include "ivf_core.h"
#include "ivf_device_rows.h"
#include "ivf_flat_lists.h"

namespace {

typedef _Float16 half2v __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------
// ranges
// ---------------------------------------------------------------------------------------------
constexpr int RANGE_ROWS = 256;  // rows per workgroup of range_kernel

// kmin[c] / kmax[c]: the smallest / largest f2key of component c over the rows (armed with 0xffffffff / 0).  Thread t
// takes components t, t + 256: a wave reads 64 adjacent halves of a row.  A NaN raises kmax to the key of a NaN.
__global__ __launch_bounds__(256) void range_kernel(const _Float16 *__restrict__ flat, int64_t n, int d, uint32_t *__restrict__ kmin,
                                                    uint32_t *__restrict__ kmax) {
  const int64_t r0 = (int64_t)blockIdx.x * RANGE_ROWS, r1 = r0 + RANGE_ROWS < n ? r0 + RANGE_ROWS : n;
  for (int c = threadIdx.x; c < d; c += 256) {
    float mn = INFINITY, mx = -INFINITY;
    bool nan = false;
    for (int64_t r = r0; r < r1; ++r) {
      const float v = (float)flat[(size_t)r * d + c];
      mn = v < mn ? v : mn;
      mx = v > mx ? v : mx;
      nan |= !(v == v);
    }
    if (r1 > r0) {
      atomicMin(&kmin[c], f2key(mn));
      atomicMax(&kmax[c], nan ? 0xffffffffu : f2key(mx));
    }
  }
}
// the keys -> vmin and vdiff = fl32(vmax - vmin); a zero minimum or maximum is +0
__global__ void range_finish_kernel(const uint32_t *__restrict__ kmin, const uint32_t *__restrict__ kmax, int d,
                                    float *__restrict__ vmin, float *__restrict__ vdiff) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= d) return;
  const float mn = key2f(kmin[c]) + 0.0f, mx = key2f(kmax[c]) + 0.0f;
  vmin[c] = mn;
  vdiff[c] = mx - mn;
}

// ---------------------------------------------------------------------------------------------
// the encoder: m prepared rows -> their codes and |xhat|^2.  One wave per row.
// ---------------------------------------------------------------------------------------------
__global__ void sq_encode_kernel(const _Float16 *__restrict__ flat, int64_t m, int d, const float *__restrict__ vmin,
                                 const float *__restrict__ step, uint8_t *__restrict__ codes, float *__restrict__ xsq) {
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= m) return;
  double ss = 0;
  for (int k = lane; k < d; k += 64) {
    const float x = (float)flat[(size_t)row * d + k], lo = vmin[k], st = step[k];
    float code = 0.0f;
    if (st != 0.0f) {
      const float t = floorf((x - lo) / st);  // two fp32 operations, each rounded once (-ffp-contract=off)
      code = t >= 0.0f ? (t < 255.0f ? t : 255.0f) : 0.0f;
    }
    codes[(size_t)row * d + k] = (uint8_t)code;
    const double xhat = (double)lo + ((double)code + 0.5) * (double)st;
    ss += xhat * xhat;
  }
  ss = wave_sum(ss);
  if (lane == 0) xsq[row] = (float)ss;
}

// byte offset, inside a 32-row block of S k-steps, of the 8 bytes lane `l` owns in k-step s (the layout at the top)
__host__ __device__ __forceinline__ size_t frag_offset(int S, int s, int l) {
  if (s < (S & ~1)) return (size_t)(s >> 1) * 1024 + (size_t)l * 16 + (size_t)(s & 1) * 8;
  return (size_t)(S >> 1) * 1024 + (size_t)l * 8;
}

// list construction: row j of the (cell, id) order goes to its list's next slot, its codes as an A fragment.  One wave per row.
__global__ void sq_scatter_kernel(const uint8_t *__restrict__ codes, const float *__restrict__ xsq, int64_t n, int d, int metric,
                                  const uint32_t *__restrict__ cell_sorted, const uint32_t *__restrict__ ord,
                                  const uint32_t *__restrict__ perm, const uint32_t *__restrict__ start,
                                  const uint32_t *__restrict__ boff, uint8_t *__restrict__ lc, float *__restrict__ lbias,
                                  uint32_t *__restrict__ lrank) {
  const int64_t j = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (j >= n) return;
  const uint32_t c = cell_sorted[j], rank = ord[j], src = perm[rank];
  const size_t slot = (size_t)boff[c] * 32 + (size_t)(j - start[c]);
  const size_t g = slot >> 5;
  const int r = (int)(slot & 31), S = d >> 4;
  for (int p = lane; p < (d >> 3); p += 64) {
    const int s = p >> 1, h = p & 1;
    *(uint2 *)&lc[g * 32 * (size_t)d + frag_offset(S, s, h * 32 + r)] = *(const uint2 *)&codes[(size_t)src * d + p * 8];
  }
  if (lane == 0) {
    lbias[slot] = metric == IVF_METRIC_L2 ? -0.5f * xsq[src] : 0.0f;
    lrank[slot] = rank;
  }
}

// ---------------------------------------------------------------------------------------------
// the queries of a chunk: fp16 rows -> s = fp16(fl32(q * step)) as B fragments ([q / 32][k-step][lane (q % 32, h)][8
// halves], frag_rows_kernel's order) and b_q = fl32(sum q (vmin + step / 2)) in fp64.  One wave per query; lane p takes
// the 8-half piece p (d / 8 <= 64 pieces).
// ---------------------------------------------------------------------------------------------
__global__ void sq_query_kernel(const _Float16 *__restrict__ q16, int nq, int d, const float *__restrict__ vmin,
                                const float *__restrict__ step, _Float16 *__restrict__ sfrag, float *__restrict__ bq) {
  const int q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int p = threadIdx.x & 63;
  if (q >= nq) return;
  double acc = 0;
  if (p < (d >> 3)) {
    const half8 v = *(const half8 *)&q16[(size_t)q * d + p * 8];
    half8 sv;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float x = (float)v[e], st = step[p * 8 + e];
      sv[e] = (_Float16)(x * st);
      acc += (double)x * ((double)vmin[p * 8 + e] + 0.5 * (double)st);
    }
    const int g = q >> 5, r = q & 31, s = p >> 1, h = p & 1;
    *(half8 *)&sfrag[((((size_t)g * (d >> 4) + s) * 64) + h * 32 + r) * 8] = sv;
  }
  acc = wave_sum(acc);
  if (p == 0) bq[q] = (float)acc;
}

// ---------------------------------------------------------------------------------------------
// the probed scan
// ---------------------------------------------------------------------------------------------
struct SqScanArgs {
  const uint8_t *lc;      // list codes, A-fragment order
  const float *lbias;     // per slot
  const uint32_t *boff;   // first block of a cell's list
  const uint32_t *nblk;   // its blocks
  const _Float16 *sf;     // the chunk's scaled queries as B fragments, S = d / 16
  const float *bq;        // [nq]
  const Group *groups;
  const uint32_t *pair_q; // queries of the pairs sorted by cell
  const float *tau;       // [nq]: emit scores >= tau; +inf = the query is finished
  uint32_t *cnt;          // [nq]
  Survivor *surv;         // [nq][CAP]
  int S;
};

// 4 code bytes -> 4 halves, exactly: the bytes (b, 0x64) are the half 1024 + b, whose ulp is 1; minus 1024 is b
__device__ __forceinline__ void bytes4_to_half4(uint32_t c, half2v &lo, half2v &hi) {
  const uint32_t a = __builtin_amdgcn_perm(0x64646464u, c, 0x04010400u);  // b0, 0x64, b1, 0x64
  const uint32_t b = __builtin_amdgcn_perm(0x64646464u, c, 0x04030402u);  // b2, 0x64, b3, 0x64
  const half2v k = {(_Float16)1024.0f, (_Float16)1024.0f};
  lo = __builtin_bit_cast(half2v, a) - k;
  hi = __builtin_bit_cast(half2v, b) - k;
}
__device__ __forceinline__ half8 bytes8_to_half8(uint32_t x, uint32_t y) {
  half2v h0, h1, h2, h3;
  bytes4_to_half4(x, h0, h1);
  bytes4_to_half4(y, h2, h3);
  return half8{h0[0], h0[1], h1[0], h1[1], h2[0], h2[1], h3[0], h3[1]};
}

__global__ __launch_bounds__(256) void sq_scan_kernel(SqScanArgs a) {
  extern __shared__ half8 sq[];  // [S][64]: the group's scaled queries as the B operand
  __shared__ int s_q[32];
  __shared__ float s_tau[32];
  __shared__ float s_bq[32];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, S = a.S;
  const Group g = a.groups[blockIdx.x];
  if (t < 32) {
    const int q = t < (int)g.count ? (int)a.pair_q[g.p0 + t] : -1;
    s_q[t] = q;
    s_tau[t] = q >= 0 ? a.tau[q] : INFINITY;
    s_bq[t] = q >= 0 ? a.bq[q] : 0.0f;
  }
  __syncthreads();
  const int myq = s_q[lane & 31];
  const float thr = s_tau[lane & 31], mybq = s_bq[lane & 31];
  if (!__syncthreads_or(thr < INFINITY)) return;  // a fallback round: every query of this group is finished
  for (int i = t; i < S * 64; i += 256) {
    const int s = i >> 6, l = i & 63, q = s_q[l & 31];
    half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (q >= 0) v = *(const half8 *)&a.sf[((((size_t)(q >> 5) * S + s) * 64) + (l >> 5) * 32 + (q & 31)) * 8];
    sq[i] = v;
  }
  __syncthreads();
  const uint32_t b0 = a.boff[g.cell], nb = a.nblk[g.cell];
  const int pairs = S >> 1;
  for (uint32_t blk = w; blk < nb; blk += 4) {
    const size_t gb = (size_t)b0 + blk;
    // row of accumulator register i on this lane: (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
    const float *bp = a.lbias + gb * 32 + 4 * (lane >> 5);
    float16v acc;
#pragma unroll
    for (int i4 = 0; i4 < 4; ++i4) {
      const float4 bv = *(const float4 *)(bp + 8 * i4);
      acc[4 * i4 + 0] = bv.x;
      acc[4 * i4 + 1] = bv.y;
      acc[4 * i4 + 2] = bv.z;
      acc[4 * i4 + 3] = bv.w;
    }
    const uint8_t *base = a.lc + gb * 512 * (size_t)S;  // 32 rows of 16 S bytes
    const uint4 *ap = (const uint4 *)base + lane;
    for (int p = 0; p < pairs; ++p) {
      const uint4 c = ap[(size_t)p * 64];
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(bytes8_to_half8(c.x, c.y), sq[(2 * p) * 64 + lane], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(bytes8_to_half8(c.z, c.w), sq[(2 * p + 1) * 64 + lane], acc, 0, 0, 0);
    }
    if (S & 1) {
      const uint2 c = *((const uint2 *)(base + (size_t)pairs * 1024) + lane);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(bytes8_to_half8(c.x, c.y), sq[(S - 1) * 64 + lane], acc, 0, 0, 0);
    }
    if (myq < 0) continue;
    // padding rows carry the bias -inf: they pass no threshold, not even -inf
    uint32_t pass = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      acc[i] += mybq;
      pass |= (uint32_t)(acc[i] >= thr && acc[i] > -INFINITY) << i;
    }
    if (pass == 0) continue;
    uint32_t pos = atomicAdd(&a.cnt[myq], (uint32_t)__popc(pass));
    const uint32_t slot0 = (uint32_t)(gb * 32) + 4u * (uint32_t)(lane >> 5);
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (pass >> i & 1) {
        if (pos < (uint32_t)CAP) a.surv[(size_t)myq * CAP + pos] = Survivor{acc[i], slot0 + (i & 3) + 8 * (i >> 2)};
        ++pos;
      }
  }
}

}  // namespace

struct ivfsq_index : IvfBase {
  // the quantiser: vmin and step on the device, vmin and vdiff as given or trained
  Buf vmin, step;
  std::vector<float> h_vmin, h_vdiff;
  // per row, in the order added
  Buf codes, xsq;
  // the lists' payload
  Buf lc, lbias;
  // per-call scratch: a slab of prepared rows; the queries, their fragments and b_q, and the groups of a search
  Buf flat, sumsq, q16, sfrag, bq;
  GroupTable gt;
};

namespace {

int new_index(int32_t device, int32_t metric, int32_t d, int32_t nlist, std::unique_ptr<ivfsq_index> &ix) {
  ITRY(hipSetDevice(device));
  ix.reset(new ivfsq_index);
  if (int rc = init_base(ix.get(), device, metric, d, nlist)) return rc;
  ITRY(ix->vmin.reserve((size_t)d * sizeof(float)));
  ITRY(ix->step.reserve((size_t)d * sizeof(float)));
  ITRY(hipFuncSetAttribute((const void *)select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SELECT_LDS));
  return IVF_OK;
}

// the host checks of a pair of ranges, which come before any device work of ivfsq_index_load
int check_ranges(int d, const float *vmin, const float *vdiff) {
  for (int i = 0; i < d; ++i) {
    if (!std::isfinite(vmin[i]) || !std::isfinite(vdiff[i])) return fail(IVF_EINVAL, "component " + std::to_string(i) + ": a range value is not finite");
    if (vdiff[i] < 0.0f) return fail(IVF_EINVAL, "component " + std::to_string(i) + ": vdiff must not be negative");
  }
  return IVF_OK;
}

// the ranges of the index: step = fl32(vdiff / 255), one IEEE division per component
int set_ranges(ivfsq_index *ix, const float *vmin, const float *vdiff) {
  const int d = ix->d;
  ix->h_vmin.assign(vmin, vmin + d);
  ix->h_vdiff.assign(vdiff, vdiff + d);
  std::vector<float> step((size_t)d);
  for (int i = 0; i < d; ++i) step[(size_t)i] = vdiff[i] / 255.0f;
  ITRY(hipMemcpy(ix->vmin.p, vmin, (size_t)d * sizeof(float), hipMemcpyHostToDevice));
  ITRY(hipMemcpy(ix->step.p, step.data(), (size_t)d * sizeof(float), hipMemcpyHostToDevice));
  return IVF_OK;
}

int build_coarse(ivfsq_index *ix, const float *h_cent, bool stored) {
  Buf cent;
  ITRY(cent.reserve((size_t)ix->nlist * ix->d * sizeof(float)));
  ITRY(hipMemcpy(cent.p, h_cent, (size_t)ix->nlist * ix->d * sizeof(float), hipMemcpyHostToDevice));
  dann_index *c = nullptr;
  DCALL(ann_by_id::dann_build_device(ix->device, ix->metric, ix->nlist, ix->d, cent.as<float>(), &c, stored));
  if (ix->coarse) (void)dann_index_destroy(ix->coarse);
  ix->coarse = c;
  return IVF_OK;
}

// all lists again from the codes in the order added: blocks of 32 rows as A fragments, beside the bias and the rank
int layout_lists(ivfsq_index *ix) {
  return layout_lists(ix, 32, [ix](size_t slots) -> int {
    const int d = ix->d;
    ITRY(ix->lc.reserve(slots * d));
    ITRY(ix->lbias.reserve(slots * sizeof(float)));
    ITRY(hipMemset(ix->lc.p, 0, slots * d));
    hipLaunchKernelGGL(fill_kernel, dim3(blocks_for((int64_t)slots)), dim3(256), 0, 0, ix->lbias.as<float>(), (int64_t)slots, -INFINITY);
    ITRY(hipGetLastError());
    hipLaunchKernelGGL(sq_scatter_kernel, dim3(blocks_for(ix->n, 4)), dim3(256), 0, 0, ix->codes.as<uint8_t>(), ix->xsq.as<float>(),
                       ix->n, d, ix->metric, ix->cell_sorted.as<uint32_t>(), ix->ord.as<uint32_t>(), ix->perm.as<uint32_t>(),
                       ix->start.as<uint32_t>(), ix->boff.as<uint32_t>(), ix->lc.as<uint8_t>(), ix->lbias.as<float>(),
                       ix->lrank.as<uint32_t>());
    ITRY(hipGetLastError());
    return IVF_OK;
  });
}

// the ranges of n prepared rows on the device -> vmin, vdiff on the host
int train_ranges(ivfsq_index *ix, const _Float16 *tflat, int64_t n, std::vector<float> &vmin, std::vector<float> &vdiff) {
  const int d = ix->d;
  Buf keys, out;
  ITRY(keys.reserve((size_t)2 * d * sizeof(uint32_t)));
  ITRY(out.reserve((size_t)2 * d * sizeof(float)));
  uint32_t *kmin = keys.as<uint32_t>(), *kmax = kmin + d;
  ITRY(hipMemset(kmin, 0xff, (size_t)d * sizeof(uint32_t)));
  ITRY(hipMemset(kmax, 0, (size_t)d * sizeof(uint32_t)));
  hipLaunchKernelGGL(range_kernel, dim3(blocks_for(n, RANGE_ROWS)), dim3(256), 0, 0, tflat, n, d, kmin, kmax);
  ITRY(hipGetLastError());
  hipLaunchKernelGGL(range_finish_kernel, dim3(blocks_for(d)), dim3(256), 0, 0, kmin, kmax, d, out.as<float>(), out.as<float>() + d);
  ITRY(hipGetLastError());
  vmin.resize((size_t)d);
  vdiff.resize((size_t)d);
  ITRY(hipMemcpy(vmin.data(), out.p, (size_t)d * sizeof(float), hipMemcpyDeviceToHost));
  ITRY(hipMemcpy(vdiff.data(), out.as<float>() + d, (size_t)d * sizeof(float), hipMemcpyDeviceToHost));
  return IVF_OK;
}

// One chunk of a search.  on_device / pos: where the queries are (probe_chunk).  out_on_device: out_dist / out_ids /
// out_counts are device buffers, which the select launch writes itself; otherwise it writes the index's own and
// finish_chunk brings them to the host.
int search_chunk(ivfsq_index *ix, int32_t q0, int32_t nq, const float *queries, bool on_device, const int64_t *pos, int32_t k,
                 int32_t nprobe, float *out_dist, int64_t *out_ids, int32_t *out_counts, bool out_on_device) {
  const int d = ix->d, S = d >> 4;
  hipStream_t st = 0;
  const int nq_pad = (nq + 31) / 32 * 32;
  ITRY(ix->q16.reserve((size_t)nq * d * sizeof(_Float16)));
  ITRY(ix->sfrag.reserve((size_t)nq_pad * d * sizeof(_Float16)));
  ITRY(ix->bq.reserve((size_t)nq * sizeof(float)));
  if (int rc = probe_chunk(ix, q0, nq, queries, on_device, pos, k, nprobe, ix->q16.as<_Float16>(), nullptr)) return rc;
  hipLaunchKernelGGL(sq_query_kernel, dim3(blocks_for(nq, 4)), dim3(256), 0, st, ix->q16.as<_Float16>(), nq, d, ix->vmin.as<float>(),
                     ix->step.as<float>(), ix->sfrag.as<_Float16>(), ix->bq.as<float>());
  ITRY(hipGetLastError());
  if (int rc = build_groups(ix, ix->gt)) return rc;
  const uint32_t n_groups = ix->gt.n_groups;

  // scan rounds
  SqScanArgs a;
  a.lc = ix->lc.as<uint8_t>();
  a.lbias = ix->lbias.as<float>();
  a.boff = ix->boff.as<uint32_t>();
  a.nblk = ix->nblk.as<uint32_t>();
  a.sf = ix->sfrag.as<_Float16>();
  a.bq = ix->bq.as<float>();
  a.groups = ix->gt.groups.as<Group>();
  a.pair_q = ix->pair_q_s.as<uint32_t>();
  a.tau = ix->tau.as<float>();
  a.cnt = ix->cnt.as<uint32_t>();
  a.surv = ix->surv.as<Survivor>();
  a.S = S;
  int rounds = 0;
  if (int rc = scan_rounds(ix, nq, k, [&](int, hipStream_t s) -> int {
        if (ix->n > 0 && n_groups > 0) {
          hipLaunchKernelGGL(sq_scan_kernel, dim3(n_groups), dim3(256), (size_t)S * 64 * sizeof(half8), s, a);
          ITRY(hipGetLastError());
        }
        return IVF_OK;
      }, &rounds))
    return rc;

  hipLaunchKernelGGL(select_kernel, dim3(nq), dim3(512), SELECT_LDS, st, ix->surv.as<Survivor>(), ix->done_cnt.as<uint32_t>(),
                     ix->qsumsq.as<float>(), ix->lrank.as<uint32_t>(), ix->ids_sorted.as<int64_t>(), ix->metric, k,
                     out_on_device ? out_dist : ix->o_dist.as<float>(), out_on_device ? out_ids : ix->o_ids.as<int64_t>(),
                     out_on_device ? out_counts : ix->o_cnt.as<int32_t>());
  ITRY(hipGetLastError());
  if (out_on_device) return finish_chunk(ix, nq, k, rounds, nullptr, nullptr, nullptr);
  return finish_chunk(ix, nq, k, rounds, out_dist, out_ids, out_counts);
}

// ivfsq_search, over host queries into host buffers or over device queries into device buffers; pos != NULL: the device
// queries are the rows pos[0 .. nq) of the store whose first row is `queries` (probe_chunk), a chunk's positions at pos + q0
int search_rows(ivfsq_index *ix, int32_t nq, const float *queries, int32_t k, int32_t nprobe, float *out_dist, int64_t *out_ids,
                int32_t *out_counts, bool on_device, const int64_t *pos = nullptr) {
  if (!ix || !queries || !out_dist || !out_ids || !out_counts) return fail(IVF_EINVAL, "null argument");
  if (int rc = search_begin(ix, nq, k, &nprobe)) return rc;
  return search_chunks(ix, nq, [&](int32_t q0, int32_t m) -> int {
    return search_chunk(ix, q0, m, pos ? queries : queries + (size_t)q0 * ix->d, on_device, pos ? pos + q0 : nullptr, k, nprobe,
                        out_dist + (size_t)q0 * k, out_ids + (size_t)q0 * k, out_counts + q0, on_device);
  });
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// the device-rows seam (ivf_device_rows.h)
// ---------------------------------------------------------------------------------------------
int ivfsq_internal::search_device_out(ivfsq_index *ix, int32_t nq, const float *d_queries, int32_t k, int32_t nprobe, float *d_dist,
                                      int64_t *d_ids, int32_t *d_counts) try {
  return search_rows(ix, nq, d_queries, k, nprobe, d_dist, d_ids, d_counts, true);
} ABI_CATCH

int ivfsq_internal::search_store_out(ivfsq_index *ix, int32_t nq, const float *d_store_rows, const int64_t *d_pos, int32_t k,
                                     int32_t nprobe, float *d_dist, int64_t *d_ids, int32_t *d_counts) try {
  if (!d_pos) return fail(IVF_EINVAL, "null argument");
  return search_rows(ix, nq, d_store_rows, k, nprobe, d_dist, d_ids, d_counts, true, d_pos);
} ABI_CATCH

int ivfsq_internal::device_of(const ivfsq_index *ix) { return ix->device; }
int64_t ivfsq_internal::last_control_bytes(const ivfsq_index *ix) { return ix->last_ctl; }
int64_t ivfsq_internal::last_control_upload_bytes(const ivfsq_index *ix) { return ix->last_ctl_up; }
std::shared_ptr<void> &ivfsq_internal::by_id_scratch(ivfsq_index *ix) { return ix->by_id; }

extern "C" {

const char *ivfsq_last_error(void) { return g_err.c_str(); }

int ivfsq_index_load(int32_t device, int32_t metric, int32_t d, int32_t nlist, const float *centroids, const float *vmin,
                     const float *vdiff, ivfsq_index_t **out) try {
  if (!centroids || !vmin || !vdiff || !out) return fail(IVF_EINVAL, "null argument");
  if (int rc = check_shape(metric, d, nlist)) return rc;
  if (int rc = check_ranges(d, vmin, vdiff)) return rc;
  std::unique_ptr<ivfsq_index> ix;
  if (int rc = new_index(device, metric, d, nlist, ix)) return rc;
  if (int rc = build_coarse(ix.get(), centroids, false)) return rc;
  if (int rc = set_ranges(ix.get(), vmin, vdiff)) return rc;
  *out = ix.release();
  return IVF_OK;
} ABI_CATCH

int ivfsq_index_train(int32_t device, int32_t metric, int32_t d, int32_t nlist, int64_t n_train, const float *train_vectors,
                      int32_t niter, uint64_t seed, ivfsq_index_t **out) try {
  if (!train_vectors || !out) return fail(IVF_EINVAL, "null argument");
  if (int rc = check_shape(metric, d, nlist)) return rc;
  if (n_train < nlist) return fail(IVF_EINVAL, "n_train must be at least nlist");
  if (n_train >= ((int64_t)1 << 31)) return fail(IVF_EINVAL, "n_train out of range");
  if (niter < -1) return fail(IVF_EINVAL, "niter must be -1 (initial picks), 0 (20 rounds) or a number of rounds");
  // the coarse quantizer, trained as an IVF-Flat index trains it
  std::vector<float> centroids((size_t)nlist * d);
  {
    ivf_index_t *flat = nullptr;
    if (int rc = ivf_index_train(device, metric, d, nlist, n_train, train_vectors, niter, seed, &flat))
      return fail(rc, std::string("coarse training: ") + ivf_last_error());
    const int rc = ivf_index_get_centroids(flat, centroids.data());
    const std::string msg = rc ? ivf_last_error() : "";
    (void)ivf_index_destroy(flat);
    if (rc) return fail(rc, "coarse training: " + msg);
  }
  std::unique_ptr<ivfsq_index> ix;
  if (int rc = new_index(device, metric, d, nlist, ix)) return rc;
  if (int rc = build_coarse(ix.get(), centroids.data(), true)) return rc;  // (the values an index stored: kept as they are)
  // the training rows, prepared as stored rows are; they go with this call
  Buf tflat, tsumsq;
  ITRY(tflat.reserve((size_t)n_train * d * sizeof(_Float16)));
  ITRY(tsumsq.reserve((size_t)n_train * sizeof(float)));
  if (int rc = upload_rows(ix.get(), train_vectors, false, n_train, tflat.as<_Float16>(), tsumsq.as<float>())) return rc;
  std::vector<float> vmin, vdiff;
  if (int rc = train_ranges(ix.get(), tflat.as<_Float16>(), n_train, vmin, vdiff)) return rc;
  for (int i = 0; i < d; ++i)
    if (!std::isfinite(vmin[(size_t)i]) || !std::isfinite(vdiff[(size_t)i]))
      return fail(IVF_EINVAL, "component " + std::to_string(i) + " of the training rows is not finite once prepared");
  if (int rc = set_ranges(ix.get(), vmin.data(), vdiff.data())) return rc;
  *out = ix.release();
  return IVF_OK;
} ABI_CATCH

int ivfsq_index_add(ivfsq_index_t *ix, int64_t n, const float *vectors, const int64_t *ids) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (n < 0) return fail(IVF_EINVAL, "n must not be negative");
  if (int rc = check_ids_rule(ix, ids != nullptr)) return rc;
  if (n == 0) return IVF_OK;
  if (!vectors) return fail(IVF_EINVAL, "null vectors");
  if (int rc = grow_rows(ix, n)) return rc;
  const int64_t n_old = ix->n, total = n_old + n;
  const int d = ix->d;
  ITRY(ix->codes.grow_keep((size_t)n_old * d, (size_t)total * d));
  ITRY(ix->xsq.grow_keep((size_t)n_old * 4, (size_t)total * 4));
  // a slab of rows at a time: prepare, assign, encode; the fp16 rows are scratch
  const int64_t slab = stage_slab_rows(d);
  ITRY(ix->flat.reserve((size_t)std::min(slab, n) * d * sizeof(_Float16)));
  ITRY(ix->sumsq.reserve((size_t)std::min(slab, n) * sizeof(float)));
  for (int64_t r0 = 0; r0 < n; r0 += slab) {
    const int64_t m = std::min(slab, n - r0), at = n_old + r0;
    if (int rc = stage_rows(ix, vectors + r0 * d, m)) return rc;
    if (int rc = prepare_slab(ix, ix->stage.as<float>(), m, ix->flat.as<_Float16>(), ix->sumsq.as<float>())) return rc;
    if (int rc = assign_rows(ix, ix->flat.as<_Float16>(), ix->sumsq.as<float>(), m, ix->cell.as<int32_t>() + at)) return rc;
    hipLaunchKernelGGL(sq_encode_kernel, dim3(blocks_for(m, 4)), dim3(256), 0, 0, ix->flat.as<_Float16>(), m, d, ix->vmin.as<float>(),
                       ix->step.as<float>(), ix->codes.as<uint8_t>() + (size_t)at * d, ix->xsq.as<float>() + at);
    ITRY(hipGetLastError());
    ITRY(hipDeviceSynchronize());
  }
  if (int rc = commit_add(ix, n, ids)) return rc;
  return layout_lists(ix);
} ABI_CATCH

int ivfsq_search(ivfsq_index_t *ix, int32_t nq, const float *queries, int32_t k, int32_t nprobe, float *out_dist, int64_t *out_ids,
                 int32_t *out_counts) try {
  return search_rows(ix, nq, queries, k, nprobe, out_dist, out_ids, out_counts, false);
} ABI_CATCH

int ivfsq_index_info(const ivfsq_index_t *ix, int64_t *n, int32_t *d, int32_t *metric, int32_t *nlist) try {
  return index_info(ix, n, d, metric, nlist);
} ABI_CATCH

int ivfsq_index_get_centroids(const ivfsq_index_t *ix, float *out) try { return get_centroids(ix, out); } ABI_CATCH

int ivfsq_index_get_ranges(const ivfsq_index_t *ix, float *vmin, float *vdiff) try {
  if (!ix) return fail(IVF_EINVAL, "null index");
  if (vmin) std::copy(ix->h_vmin.begin(), ix->h_vmin.end(), vmin);
  if (vdiff) std::copy(ix->h_vdiff.begin(), ix->h_vdiff.end(), vdiff);
  return IVF_OK;
} ABI_CATCH

int ivfsq_index_list_sizes(const ivfsq_index_t *ix, int64_t *out) try { return list_sizes(ix, out); } ABI_CATCH

int ivfsq_index_get_assignment(const ivfsq_index_t *ix, int64_t *out_ids, int32_t *out_cells) try {
  return get_assignment(ix, out_ids, out_cells);
} ABI_CATCH

int ivfsq_index_get_codes(const ivfsq_index_t *ix, int64_t r0, int64_t m, uint8_t *out) try {
  if (!ix || !out) return fail(IVF_EINVAL, "null argument");
  return export_columns(ix, r0, m, nullptr, nullptr, out, ix->codes.p, (size_t)ix->d);
} ABI_CATCH

int ivfsq_last_probes(const ivfsq_index_t *ix, int32_t *nq, int32_t *nprobe, int32_t *out_cells) try {
  return last_probes(ix, nq, nprobe, out_cells);
} ABI_CATCH

int ivfsq_last_stats(const ivfsq_index_t *ix, int64_t *rows_scanned, int32_t *rounds, float *coarse_ms, float *scan_ms,
                     float *select_ms) try {
  return last_stats(ix, rows_scanned, rounds, coarse_ms, scan_ms, select_ms);
} ABI_CATCH

int ivfsq_index_destroy(ivfsq_index_t *ix) try {
  delete ix;
  return IVF_OK;
} ABI_CATCH

}  // extern "C"
