// row_score.h -- the distance of a (query, stored fp16 row) pair on the device, which the re-rank (refine_ann.hip) and the
// Annoy index (annoy_ann.hip: its re-score, and the loads and the wave sum of its margin) share, and the emit of the answer
// from sorted keys.  The two must agree bit for bit; every byte golden and the host's emulated margin
// (annoy_forest.h::margin) rest on the order stated here.
//
// The store is fp16 [n][stride], stride = d rounded up to 8 halves (16 bytes), the padding zero; a query is prepared as a
// row is.  Row and query are cut into `pieces` = stride / 8 pieces of 8 components.  Lane l of a 64-lane wave owns pieces
// l and l + 64 (NP = 1: stride <= 512, NP = 2: stride <= 1024); a lane without a piece holds zeros.  All arithmetic is fp32
// and unfused (the including files are compiled with -ffp-contract=off): a lane starts from 0 and adds, piece l before piece
// l + 64 and within a piece components 0..7, t * t with t = q_i - x_i (L2) or q_i * x_i (otherwise); the 64 lane sums meet
// in the xor tree o = 32, 16, 8, 4, 2, 1; the distance is sqrtf of that (L2) or 1 - that.  A wave scores ROWS_IN_FLIGHT rows
// at a time: every load is issued before the first add.
//
// A source includes this once; everything is file-local.  Nothing here knows its caller.
#pragma once
#include "survivor_topk.h"  // half8, f2key, key2f, sort_keys_desc

namespace {

constexpr int ROWS_IN_FLIGHT = 4;

// this lane's pieces of one row of `pieces` pieces: zeros past the row's end, and for a row that is not there
template <int NP>
__device__ __forceinline__ void load_pieces(const _Float16 *row, bool present, int pieces, half8 (&x)[NP]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int p = lane + 64 * j;
    half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (present && p < pieces) v = *(const half8 *)(row + p * 8);
    x[j] = v;
  }
}

// this lane's pieces of a prepared query, widened
template <int NP>
__device__ __forceinline__ void load_query(const _Float16 *q, int pieces, float (&qf)[NP][8]) {
  half8 v[NP];
  load_pieces<NP>(q, true, pieces, v);
#pragma unroll
  for (int j = 0; j < NP; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) qf[j][i] = (float)v[j][i];
}

// the xor tree over a wave's 64 fp32 lane sums: every lane ends with the same bits
__device__ __forceinline__ float wave_sum_f32(float acc) {
  for (int o = 32; o; o >>= 1) acc += __shfl_xor(acc, o, 64);
  return acc;
}

// the distances of the query in qf to the rows at pos[0..ROWS_IN_FLIGHT) of the store (a negative position: no row, and a
// distance that means nothing), the same in every lane
template <int NP>
__device__ __forceinline__ void score_rows(const _Float16 *rows, int stride, int pieces, const int64_t (&pos)[ROWS_IN_FLIGHT],
                                           const float (&qf)[NP][8], bool l2, float (&dist)[ROWS_IN_FLIGHT]) {
  half8 x[ROWS_IN_FLIGHT][NP];
#pragma unroll
  for (int u = 0; u < ROWS_IN_FLIGHT; ++u) load_pieces<NP>(rows + (size_t)pos[u] * stride, pos[u] >= 0, pieces, x[u]);
#pragma unroll
  for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < NP; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xv = (float)x[u][j][e];
        if (l2) {
          const float df = qf[j][e] - xv;
          acc += df * df;
        } else {
          acc += qf[j][e] * xv;
        }
      }
    acc = wave_sum_f32(acc);
    dist[u] = l2 ? sqrtf(acc) : 1.0f - acc;
  }
}

// One query's answer from its workgroup's LDS keys, sorted by sort_keys_desc as complements of f2key(dist) << 32 | rank:
// the first m of them, then 0 / 0 up to k; a key whose complement is ~0 (no candidate) is written as 0 / 0 too.  out_dist
// and out_ids are the query's k slots, out_count its count.
__device__ __forceinline__ void emit_sorted(const unsigned long long *keys, uint32_t m, int k, const int64_t *ids_sorted,
                                            float *out_dist, int64_t *out_ids, int32_t *out_count) {
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    float dist = 0.0f;
    int64_t id = 0;
    if ((uint32_t)i < m) {
      const unsigned long long key = ~keys[i];
      if (key != ~0ull) {
        dist = key2f((uint32_t)(key >> 32));
        id = ids_sorted[(uint32_t)key];
      }
    }
    out_dist[i] = dist;
    out_ids[i] = id;
  }
  if (threadIdx.x == 0) *out_count = (int32_t)m;
}

}  // namespace
