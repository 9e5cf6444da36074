// ivf_flat_lists.h -- the payload scatter and the select step of flat (fp16-row) lists, shared by the two indexes whose
// lists hold rows as MFMA A fragments: ivf_ann.hip (cell = nearest centroid) and grouped_ann.hip (cell = the caller's
// group); and the group table of a search chunk, shared by ivf_ann.hip and ivfsq_ann.hip (whose lists hold code bytes in
// the same fragment order and whose answers go through the same select step).  A source includes this once, after
// ivf_core.h.  Everything is file-local.
#pragma once
#include "ivf_core.h"

namespace {

// ---------------------------------------------------------------------------------------------
// list construction: row j of the (cell, id) order goes to its list's next slot, as an A fragment.  One wave per row.
// ---------------------------------------------------------------------------------------------
__global__ void scatter_rows_kernel(const _Float16 *__restrict__ flat, const float *__restrict__ sumsq, int64_t n, int d,
                                    int metric, const uint32_t *__restrict__ cell_sorted, const uint32_t *__restrict__ ord,
                                    const uint32_t *__restrict__ perm, const uint32_t *__restrict__ start,
                                    const uint32_t *__restrict__ boff, _Float16 *__restrict__ lf, float *__restrict__ lbias,
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
    *(half8 *)&lf[(((g * S + s) * 64) + h * 32 + r) * 8] = *(const half8 *)&flat[(size_t)src * d + p * 8];
  }
  if (lane == 0) {
    lbias[slot] = metric == IVF_METRIC_L2 ? -0.5f * sumsq[src] : 0.0f;
    lrank[slot] = rank;
  }
}

// ---------------------------------------------------------------------------------------------
// the group table of a chunk, for the scans that run one workgroup per Group (ivf_ann.hip, ivfsq_ann.hip): after
// probe_chunk, the pairs of a cell cut into groups of <= 32 queries; the rows scanned are counted into rows_acc.
// ---------------------------------------------------------------------------------------------
struct GroupTable {
  Buf pstart, ngrp, gstart, groups;
  uint32_t n_groups = 0;
};
int build_groups(IvfBase *ix, GroupTable &gt) {
  const int nlist = ix->nlist;
  hipStream_t st = 0;
  ITRY(gt.pstart.reserve((size_t)nlist * 4));
  ITRY(gt.ngrp.reserve((size_t)nlist * 4));
  ITRY(gt.gstart.reserve((size_t)nlist * 4));
  hipLaunchKernelGGL(blocks_of_kernel, dim3(blocks_for(nlist)), dim3(256), 0, st, ix->per_cell.as<uint32_t>(), nlist, 32u,
                     gt.ngrp.as<uint32_t>());
  ITRY(hipGetLastError());
  if (int rc = exclusive_sum(ix, ix->per_cell.as<uint32_t>(), gt.pstart.as<uint32_t>(), nlist)) return rc;
  if (int rc = exclusive_sum(ix, gt.ngrp.as<uint32_t>(), gt.gstart.as<uint32_t>(), nlist)) return rc;
  uint32_t last[2] = {0, 0};
  ITRY(hipMemcpy(&last[0], gt.gstart.as<uint32_t>() + (nlist - 1), 4, hipMemcpyDeviceToHost));
  ITRY(hipMemcpy(&last[1], gt.ngrp.as<uint32_t>() + (nlist - 1), 4, hipMemcpyDeviceToHost));
  gt.n_groups = last[0] + last[1];
  ix->last_ctl += 8;
  ITRY(gt.groups.reserve((size_t)gt.n_groups * sizeof(Group)));
  hipLaunchKernelGGL(groups_kernel, dim3(blocks_for(nlist)), dim3(256), 0, st, ix->per_cell.as<uint32_t>(), gt.pstart.as<uint32_t>(),
                     gt.gstart.as<uint32_t>(), ix->sizes.as<uint32_t>(), nlist, gt.groups.as<Group>(),
                     ix->rows_acc.as<unsigned long long>());
  ITRY(hipGetLastError());
  return IVF_OK;
}

// per query: sort survivors by (score desc, rank in id order asc), emit the k nearest as distances (dense_ann.hip's select
// with the list slot in place of the position)
__global__ __launch_bounds__(512) void select_kernel(const Survivor *__restrict__ surv, const uint32_t *__restrict__ done_cnt,
                                                     const float *__restrict__ qsumsq, const uint32_t *__restrict__ lrank,
                                                     const int64_t *__restrict__ ids_sorted, int metric, int k,
                                                     float *__restrict__ out_dist, int64_t *__restrict__ out_ids,
                                                     int32_t *__restrict__ out_counts) {
  extern __shared__ unsigned long long keys[];
  const int q = blockIdx.x;
  const uint32_t c = select_sorted(surv, done_cnt, lrank, q, keys);
  const uint32_t m = min(c, (uint32_t)k);
  for (uint32_t i = threadIdx.x; i < (uint32_t)k; i += blockDim.x) {
    float dist = 0.0f;
    int64_t id = 0;
    if (i < m) {
      unsigned long long key = keys[i];
      float sc = key2f((uint32_t)(key >> 32));
      id = ids_sorted[0xffffffffu - (uint32_t)key];
      if (metric == IVF_METRIC_L2) dist = sqrtf(fmaxf(0.0f, qsumsq[q] - 2.0f * sc));
      else dist = 1.0f - sc;
    }
    out_dist[(size_t)q * k + i] = dist;
    out_ids[(size_t)q * k + i] = id;
  }
  if (threadIdx.x == 0) out_counts[q] = (int32_t)m;
}

}  // namespace
