// by_id_core.h -- what the two by-id sources share (ann_by_id.hip: the dense indexes of include/ann_by_id.h; faiss_by_id.hip:
// the inverted-file family and shard sets of include/faiss_by_id.h): the first and the last step of a by-id query and the
// scratch they run in.
//   resolve   the seed ids are uploaded (8 bytes each), each looks itself up in the producer's (key, position) table sorted by
//             key, and an exclusive scan of the found flags gives every found seed its compact query slot
//   flatten   an exclusive scan of the per-seed counts, then one wave per seed writes its (seed, id, distance) triples at its
//             offset -- the counts may differ from seed to seed, the rows are packed; out_total triples and the counts are all
//             that is copied back
// The status codes are ANN_BY_ID_* (the numbers every index module shares).  A source includes this once, after nothing that
// defines BTRY; everything is file-local, so each source has its own g_err behind its own *_last_error().
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>
#include <memory>
#include <string>

#include "../../include/ann_by_id.h"
#include "device_buf.h"
#include "host_error.h"
#define BTRY(expr) HIP_TRY_AS(ANN_BY_ID_EDEVICE, expr)

namespace {

// ---- kernels ---------------------------------------------------------------------------------------------------------

// Resolve: pos[i] = the producer's row of seed i (-1: absent), flag[i] = found.  positional: the keys are positions 0..nt-1.
__global__ void by_id_resolve_kernel(const int64_t *__restrict__ keys, const int64_t *__restrict__ kpos, int64_t nt, int positional,
                                     const int64_t *__restrict__ seeds, int64_t n, int64_t *__restrict__ pos,
                                     int32_t *__restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t k = seeds[i];
  int64_t p = -1;
  if (positional) {
    if (k >= 0 && k < nt) p = k;
  } else {
    int64_t lo = 0, hi = nt;  // lower_bound
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (keys[mid] < k) lo = mid + 1;
      else hi = mid;
    }
    if (lo < nt && keys[lo] == k) p = kpos[lo];
  }
  pos[i] = p;
  flag[i] = p >= 0 ? 1 : 0;
}

// per-seed neighbour counts for the scan (0 for an absent seed); counts == NULL: a search that answers nothing
__global__ void by_id_seed_counts_kernel(const int32_t *__restrict__ flag, const int32_t *__restrict__ slot,
                                         const int32_t *__restrict__ counts, int64_t n, int32_t *__restrict__ c) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  c[i] = i < n && flag[i] && counts ? counts[slot[i]] : 0;  // (entry n: the scan's total)
}

// One wave per seed: its triples at its offset, and its count (-1: absent).
__global__ __launch_bounds__(256) void by_id_flatten_kernel(const int64_t *__restrict__ seeds, const int32_t *__restrict__ flag,
                                                            const int32_t *__restrict__ slot, const int32_t *__restrict__ c,
                                                            const int32_t *__restrict__ off, int64_t n, int k,
                                                            const float *__restrict__ dist, const int64_t *__restrict__ ids,
                                                            int64_t *__restrict__ o_seed, int64_t *__restrict__ o_id,
                                                            float *__restrict__ o_dist, int32_t *__restrict__ o_counts) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= n) return;
  const bool found = flag[i] != 0;
  if (lane == 0) o_counts[i] = found ? c[i] : -1;
  if (!found) return;
  const int cnt = c[i];
  const int64_t at = off[i], from = (int64_t)slot[i] * k;
  const int64_t seed = seeds[i];
  for (int j = lane; j < cnt; j += 64) {
    o_seed[at + j] = seed;
    o_id[at + j] = ids[from + j];
    o_dist[at + j] = dist[from + j];
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------

// Per-index scratch and the last call's figures (kept on the index handle: one call at a time per index).
struct Scratch {
  Buf seeds, pos, flag, slot, c, off, scan_tmp, f_seed, f_id, f_dist, f_counts, r_dist, r_ids, r_cnt;
  Buf qpos;  // faiss_by_id.hip: the positions of the found seeds in request order
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  int64_t found = 0, absent = 0, h2d = 0, d2h = 0, d2h_result = 0;
  float t_gather = 0, t_search = 0, t_flatten = 0;
  ~Scratch() {
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

int get_scratch(std::shared_ptr<void> &slot, Scratch **out) {
  if (!slot) {
    auto s = std::make_shared<Scratch>();
    for (auto &e : s->ev) BTRY(hipEventCreate(&e));
    slot = s;
  }
  *out = static_cast<Scratch *>(slot.get());
  return ANN_BY_ID_OK;
}

// The producer's (key, position) table of a call.
struct KeyTable {
  const int64_t *keys = nullptr, *kpos = nullptr;
  int64_t nt = 0;
  bool positional = false;  // the keys are the positions 0..nt-1 (an index created without ids as its own producer)
};

int check_common(const void *index, int32_t n_seeds, const int64_t *seeds, int64_t *out_seed, int64_t *out_id, float *out_dist,
                 int64_t cap, int64_t *out_total, int32_t *out_counts) {
  if (n_seeds < 0 || n_seeds >= 0x7fffffff) return fail(ANN_BY_ID_EINVAL, "n_seeds out of range");
  if (cap < 0) return fail(ANN_BY_ID_EINVAL, "cap must not be negative");
  if (!index || !out_total || (n_seeds > 0 && (!seeds || !out_counts)) || (cap > 0 && (!out_seed || !out_id || !out_dist)))
    return fail(ANN_BY_ID_EINVAL, "NULL argument");
  return ANN_BY_ID_OK;
}

// Step 1: upload, resolve, scan.  Leaves s->found / absent; the first event is recorded before the upload.
int resolve(Scratch *s, const KeyTable &p, int32_t n, const int64_t *seeds) {
  hipStream_t st = 0;
  s->found = s->absent = s->h2d = s->d2h = s->d2h_result = 0;
  s->t_gather = s->t_search = s->t_flatten = 0;
  BTRY(s->seeds.reserve((size_t)n * 8));
  BTRY(s->pos.reserve((size_t)n * 8));
  BTRY(s->flag.reserve(((size_t)n + 1) * 4));
  BTRY(s->slot.reserve(((size_t)n + 1) * 4));
  BTRY(s->c.reserve(((size_t)n + 1) * 4));
  BTRY(s->off.reserve(((size_t)n + 1) * 4));
  BTRY(s->f_counts.reserve((size_t)n * 4));
  size_t tb = 0;
  BTRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (const int32_t *)nullptr, (int32_t *)nullptr, n + 1, st));
  BTRY(s->scan_tmp.reserve(tb));
  BTRY(hipEventRecord(s->ev[0], st));
  BTRY(hipMemcpyAsync(s->seeds.p, seeds, (size_t)n * 8, hipMemcpyHostToDevice, st));
  s->h2d += (int64_t)n * 8;
  BTRY(hipMemsetAsync(s->flag.as<int32_t>() + n, 0, 4, st));
  hipLaunchKernelGGL(by_id_resolve_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p.keys, p.kpos, p.nt, p.positional ? 1 : 0, s->seeds.as<int64_t>(),
                     (int64_t)n, s->pos.as<int64_t>(), s->flag.as<int32_t>());
  BTRY(hipGetLastError());
  tb = s->scan_tmp.bytes;
  BTRY(hipcub::DeviceScan::ExclusiveSum(s->scan_tmp.p, tb, s->flag.as<int32_t>(), s->slot.as<int32_t>(), n + 1, st));
  int32_t found = 0;
  BTRY(hipMemcpyAsync(&found, s->slot.as<int32_t>() + n, 4, hipMemcpyDeviceToHost, st));
  BTRY(hipStreamSynchronize(st));
  s->d2h += 4;
  s->found = found;
  s->absent = n - found;
  return ANN_BY_ID_OK;
}

// Step 4: scan the per-seed counts, write the triples, copy out_total of them and the counts back.
int flatten(Scratch *s, int32_t n, int32_t k, const float *r_dist, const int64_t *r_ids, const int32_t *r_cnt, int64_t *out_seed,
            int64_t *out_id, float *out_dist, int64_t *out_total, int32_t *out_counts) {
  hipStream_t st = 0;
  BTRY(s->f_seed.reserve((size_t)s->found * k * 8));
  BTRY(s->f_id.reserve((size_t)s->found * k * 8));
  BTRY(s->f_dist.reserve((size_t)s->found * k * 4));
  BTRY(hipEventRecord(s->ev[2], st));
  hipLaunchKernelGGL(by_id_seed_counts_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, st, s->flag.as<int32_t>(), s->slot.as<int32_t>(),
                     r_cnt, (int64_t)n, s->c.as<int32_t>());
  BTRY(hipGetLastError());
  size_t tb = s->scan_tmp.bytes;
  BTRY(hipcub::DeviceScan::ExclusiveSum(s->scan_tmp.p, tb, s->c.as<int32_t>(), s->off.as<int32_t>(), n + 1, st));
  hipLaunchKernelGGL(by_id_flatten_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, s->seeds.as<int64_t>(), s->flag.as<int32_t>(),
                     s->slot.as<int32_t>(), s->c.as<int32_t>(), s->off.as<int32_t>(), (int64_t)n, k, r_dist, r_ids, s->f_seed.as<int64_t>(),
                     s->f_id.as<int64_t>(), s->f_dist.as<float>(), s->f_counts.as<int32_t>());
  BTRY(hipGetLastError());
  BTRY(hipEventRecord(s->ev[3], st));
  int32_t total = 0;
  BTRY(hipMemcpyAsync(&total, s->off.as<int32_t>() + n, 4, hipMemcpyDeviceToHost, st));
  BTRY(hipStreamSynchronize(st));
  s->d2h += 4;
  if (total > 0) {
    BTRY(hipMemcpyAsync(out_seed, s->f_seed.p, (size_t)total * 8, hipMemcpyDeviceToHost, st));
    BTRY(hipMemcpyAsync(out_id, s->f_id.p, (size_t)total * 8, hipMemcpyDeviceToHost, st));
    BTRY(hipMemcpyAsync(out_dist, s->f_dist.p, (size_t)total * 4, hipMemcpyDeviceToHost, st));
  }
  BTRY(hipMemcpyAsync(out_counts, s->f_counts.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  BTRY(hipStreamSynchronize(st));
  s->d2h_result = (int64_t)total * 20 + (int64_t)n * 4;
  s->d2h += s->d2h_result;
  *out_total = total;
  (void)hipEventElapsedTime(&s->t_flatten, s->ev[2], s->ev[3]);
  return ANN_BY_ID_OK;
}

int cap_check(const Scratch *s, int32_t k, int64_t cap) {
  if (s->found * k >= (int64_t)0x7fffffff) return fail(ANN_BY_ID_ELIMIT, "n_found * k reaches 2^31 - 1 triples");
  if (cap < s->found * k)
    return fail(ANN_BY_ID_EINVAL, "cap " + std::to_string(cap) + " is below n_found * k = " + std::to_string(s->found) + " * " + std::to_string(k));
  return ANN_BY_ID_OK;
}

}  // namespace
