// sann_wave.h -- wave64 primitives on the VALU for gfx950: DPP reductions / scans, lane exchange without the LDS
// crossbar, and in-register bitonic sorts (one value per lane).  Shared by the unit kernel and the merge kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// The lane number the helpers below branch on.  A kernel whose body is one big LOOP can define it, before this header is
// included, as something the optimiser cannot prove loop-invariant: the dozens of lane predicates of the sort networks are
// otherwise hoisted out of the loop and held in SGPR pairs for the kernel's whole life (round 3's pipelined unit kernel: 97
// spilled SGPRs; profiles/r03_pipelined_unit_kernel_experiment.txt).
#ifndef SANN_WAVE_LANE
#define SANN_WAVE_LANE() ((int)(threadIdx.x & 63))
#endif

namespace sann {

// ---------------------------------------------------------------------------------------------
// wave64 reductions on the VALU (DPP), result valid in every lane after the readlane
// ---------------------------------------------------------------------------------------------
template <int CTRL, int ROW_MASK>
__device__ inline uint32_t dpp_u32(uint32_t old, uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ inline uint32_t wave_max_u32(uint32_t v) {
  v = max(v, dpp_u32<0xB1, 0xf>(0u, v));   // quad_perm [1,0,3,2]
  v = max(v, dpp_u32<0x4E, 0xf>(0u, v));   // quad_perm [2,3,0,1]
  v = max(v, dpp_u32<0x124, 0xf>(0u, v));  // row_ror 4
  v = max(v, dpp_u32<0x128, 0xf>(0u, v));  // row_ror 8
  v = max(v, dpp_u32<0x142, 0xa>(0u, v));  // row_bcast 15 -> rows 1,3
  v = max(v, dpp_u32<0x143, 0xc>(0u, v));  // row_bcast 31 -> rows 2,3
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ inline uint32_t wave_min_u32(uint32_t v) { return ~wave_max_u32(~v); }
// inclusive prefix sum over the wave, on the VALU (DPP row shifts, then the two row broadcasts)
__device__ inline int wave_incl_scan_i32(int x) {
  uint32_t v = (uint32_t)x;
  v += dpp_u32<0x111, 0xf>(0u, v);  // row_shr:1
  v += dpp_u32<0x112, 0xf>(0u, v);  // row_shr:2
  v += dpp_u32<0x114, 0xf>(0u, v);  // row_shr:4
  v += dpp_u32<0x118, 0xf>(0u, v);  // row_shr:8
  v += dpp_u32<0x142, 0xa>(0u, v);  // row_bcast:15 -> rows 1, 3
  v += dpp_u32<0x143, 0xc>(0u, v);  // row_bcast:31 -> rows 2, 3
  return (int)v;
}

// Value of lane (l ^ J), without a trip through the LDS crossbar (a chain of 21 ds_bpermute round trips cost the
// sort below ~6k cycles of latency): quad permutes, row shifts, and gfx950's row / half-wave swaps.
template <int J>
__device__ inline uint32_t lane_xor(uint32_t v) {
  const int lane = SANN_WAVE_LANE();
  if constexpr (J == 1) return dpp_u32<0xB1, 0xf>(v, v);  // quad_perm [1,0,3,2]
  else if constexpr (J == 2) return dpp_u32<0x4E, 0xf>(v, v);  // quad_perm [2,3,0,1]
  else if constexpr (J == 4 || J == 8) {
    const uint32_t up = dpp_u32<0x100 + J, 0xf>(v, v);    // row_shl:J  -> lane l reads l + J
    const uint32_t down = dpp_u32<0x110 + J, 0xf>(v, v);  // row_shr:J  -> lane l reads l - J
    return (lane & J) ? down : up;
  } else if constexpr (J == 16) {
    const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);  // r[0] = rows (0,0,2,2), r[1] = rows (1,1,3,3)
    return (lane & 16) ? r[0] : r[1];
  } else {
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);  // r[0] = halves (lo,lo), r[1] = (hi,hi)
    return (lane & 32) ? r[0] : r[1];
  }
}
template <int K, int J>
__device__ inline uint32_t bitonic_step(uint32_t v) {
  const int lane = SANN_WAVE_LANE();
  const uint32_t o = lane_xor<J>(v);
  const bool keep_max = ((lane & K) == 0) == ((lane & J) == 0);
  return keep_max ? (v > o ? v : o) : (v < o ? v : o);
}
// bitonic sort of one value per lane, descending: lane i ends up with the wave's i-th largest
__device__ inline uint32_t wave_sort_desc_u32(uint32_t v) {
  v = bitonic_step<2, 1>(v);
  v = bitonic_step<4, 2>(v); v = bitonic_step<4, 1>(v);
  v = bitonic_step<8, 4>(v); v = bitonic_step<8, 2>(v); v = bitonic_step<8, 1>(v);
  v = bitonic_step<16, 8>(v); v = bitonic_step<16, 4>(v); v = bitonic_step<16, 2>(v); v = bitonic_step<16, 1>(v);
  v = bitonic_step<32, 16>(v); v = bitonic_step<32, 8>(v); v = bitonic_step<32, 4>(v); v = bitonic_step<32, 2>(v); v = bitonic_step<32, 1>(v);
  v = bitonic_step<64, 32>(v); v = bitonic_step<64, 16>(v); v = bitonic_step<64, 8>(v); v = bitonic_step<64, 4>(v); v = bitonic_step<64, 2>(v); v = bitonic_step<64, 1>(v);
  return v;
}


// ---- 128-bit keys (hi, lo), one per lane: the merge kernel's (score key, id key) ---------------------------------------
// The network is paced by vector issue (profiles/NOTES.md, round 13), so a step spends vector instructions on three things
// only: fetching the partner's four dwords, ONE 128-bit compare, and four selects.
//   * which lanes keep the larger key is a compile-time pattern of (K, J): a 64-bit literal XOR-ed into the compare's lane
//     mask on the scalar side -- no lane arithmetic, no mask held in (or spilled from) SGPRs;
//   * `take = (other > mine) == keep_max` needs no second compare: the two lanes of a pair decide from the same two keys,
//     and on equal keys either choice exchanges identical bits;
//   * J = 1, 2, 8 are one DPP move per dword (quad permutes, row_ror:8 = l ^ 8 within a row of 16); J = 4 is two moves into
//     one register under complementary bank masks; J = 16, 32 swap two copies of the key, after which the pair
//     (r0, r1) IS (mine, other) in the even rows / the low half and (other, mine) in the others -- `r1 > r0` is then
//     "other > mine" there and its negation here, and the select `sel ? r1 : r0` with sel = (r1 > r0) ^ ~keep_max serves both.
template <int K, int J>
constexpr uint64_t bitonic_keep_max_lanes() {
  uint64_t m = 0;
  for (int l = 0; l < 64; l++)
    if (((l & K) == 0) == ((l & J) == 0)) m |= 1ull << l;
  return m;
}
// lanes where a > b over four dwords, [3] the most significant: three 64-bit compares whose lane masks meet on the scalar side
__device__ inline uint64_t k128_gt_lanes(const uint32_t (&a)[4], const uint32_t (&b)[4]) {
  const uint64_t ah = ((uint64_t)a[3] << 32) | a[2], al = ((uint64_t)a[1] << 32) | a[0];
  const uint64_t bh = ((uint64_t)b[3] << 32) | b[2], bl = ((uint64_t)b[1] << 32) | b[0];
  return __builtin_amdgcn_ballot_w64(ah > bh) | (__builtin_amdgcn_ballot_w64(ah == bh) & __builtin_amdgcn_ballot_w64(al > bl));
}
template <int K, int J>
__device__ inline void bitonic_step_k128(uint32_t (&m)[4]) {
  constexpr uint64_t FLIP = ~bitonic_keep_max_lanes<K, J>();
  uint32_t a[4], o[4];  // the select's "else" and "then" operands
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if constexpr (J == 1) {
      a[i] = m[i]; o[i] = (uint32_t)__builtin_amdgcn_mov_dpp((int)m[i], 0xB1, 0xf, 0xf, true);  // quad_perm [1,0,3,2]
    } else if constexpr (J == 2) {
      a[i] = m[i]; o[i] = (uint32_t)__builtin_amdgcn_mov_dpp((int)m[i], 0x4E, 0xf, 0xf, true);  // quad_perm [2,3,0,1]
    } else if constexpr (J == 4) {
      // row_shl:4 (lane l reads l + 4) into banks 0, 2; row_shr:4 (l - 4) into banks 1, 3: every lane is written once
      const int up = __builtin_amdgcn_mov_dpp((int)m[i], 0x104, 0xf, 0x5, false);
      a[i] = m[i]; o[i] = (uint32_t)__builtin_amdgcn_update_dpp(up, (int)m[i], 0x114, 0xf, 0xa, false);
    } else if constexpr (J == 8) {
      a[i] = m[i]; o[i] = (uint32_t)__builtin_amdgcn_mov_dpp((int)m[i], 0x128, 0xf, 0xf, true);  // row_ror:8
    } else if constexpr (J == 16) {
      const auto r = __builtin_amdgcn_permlane16_swap(m[i], m[i], false, false);  // r[0] = rows (0,0,2,2), r[1] = rows (1,1,3,3)
      a[i] = r[0]; o[i] = r[1];
    } else {
      const auto r = __builtin_amdgcn_permlane32_swap(m[i], m[i], false, false);  // r[0] = halves (lo,lo), r[1] = (hi,hi)
      a[i] = r[0]; o[i] = r[1];
    }
  }
  const bool sel = __builtin_amdgcn_inverse_ballot_w64(k128_gt_lanes(o, a) ^ FLIP);
#pragma unroll
  for (int i = 0; i < 4; i++) m[i] = sel ? o[i] : a[i];
}
// bitonic sort of one 128-bit key per lane, descending: lane i ends up with the wave's i-th largest
__device__ inline void wave_sort_desc_k128(uint64_t &hi, uint64_t &lo) {
  uint32_t m[4] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
#define S_(K, J) bitonic_step_k128<K, J>(m)
  S_(2, 1);
  S_(4, 2); S_(4, 1);
  S_(8, 4); S_(8, 2); S_(8, 1);
  S_(16, 8); S_(16, 4); S_(16, 2); S_(16, 1);
  S_(32, 16); S_(32, 8); S_(32, 4); S_(32, 2); S_(32, 1);
  S_(64, 32); S_(64, 16); S_(64, 8); S_(64, 4); S_(64, 2); S_(64, 1);
#undef S_
  lo = ((uint64_t)m[1] << 32) | m[0];
  hi = ((uint64_t)m[3] << 32) | m[2];
}

}  // namespace sann
