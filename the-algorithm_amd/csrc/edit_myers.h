// edit_myers.h -- the distance core of include/edit_ann.h: bit-parallel Levenshtein distance (Myers 1999) in the block form
// that computes the global distance, and the per-query match-mask table it reads.  Plain C++ with no device intrinsic, so
// the very function the kernels of edit_ann.hip run also compiles for the host, where tests/edit_host_check.cpp holds it
// against the plain dynamic programme.
//
// The query is the pattern: m elements in W = ceil(m / 64) words of vertical deltas Pv / Mv, score starting at m (column 0
// of the table is 0, 1, .., m).  Per text element every word takes one column step with a horizontal delta hin in {-1, 0, +1}
// coming in at its bit 0 and hout leaving at its bit 63.  hin of word 0 is +1: row 0 of the table is 0, 1, 2, ...  Inside a
// step the carry of (Eq & Pv) + Pv stays in its word: the block form accounts for what crosses a word boundary through hin
// alone (a negative hin sets bit 0 of the word's Eq for Xh).  The score moves by the Ph / Mh bit at (m - 1) mod 64 of the
// last word; the bits above it in that word hold garbage that never travels down.
//
// Equality of elements is IEEE ==: both sides are canonicalised (-0.0 -> +0.0) and compared as bits, a NaN is never
// inserted, and a NaN looked up walks to an empty slot, whose mask is zero.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EDIT_HD __host__ __device__ __forceinline__
#else
#define EDIT_HD inline
#endif
#if defined(__clang__)
#define EDIT_UNROLL _Pragma("unroll")
#else
#define EDIT_UNROLL
#endif

namespace edit_core {

constexpr int MAX_LEN = 256;
constexpr int MAX_WORDS = 4;
constexpr int TABLE_SLOTS = 512;          // open addressing, at most 256 distinct symbols: load factor <= 1/2
constexpr uint32_t EMPTY_KEY = 0xffffffffu;  // a NaN pattern: never a key

EDIT_HD uint32_t canonical(uint32_t bits) { return bits == 0x80000000u ? 0u : bits; }
EDIT_HD bool is_nan(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }
EDIT_HD uint32_t slot_of(uint32_t key) { return (key * 0x9e3779b1u) >> 23; }

// The slot that holds `key`, or the empty slot its probe sequence ends at.  keys[TABLE_SLOTS].
EDIT_HD uint32_t find_slot(const uint32_t *keys, uint32_t key) {
  uint32_t h = slot_of(key);
  for (int i = 0; i < TABLE_SLOTS; i++) {  // (bounded: the table is never full)
    const uint32_t k = keys[h];
    if (k == key || k == EMPTY_KEY) break;
    h = (h + 1) & (TABLE_SLOTS - 1);
  }
  return h;
}

// Distance of the pattern behind (keys, masks) -- m elements, masks[slot * W + w] -- to the text text[0], text[stride], ..,
// n elements of raw fp32 bits.
template <int W>
EDIT_HD int32_t distance(const uint32_t *keys, const uint64_t *masks, int m, const uint32_t *text, int64_t stride, int n) {
  uint64_t pv[W], mv[W];
EDIT_UNROLL
  for (int w = 0; w < W; w++) {
    pv[w] = ~0ull;
    mv[w] = 0;
  }
  int32_t score = m;
  const uint64_t top = 1ull << ((m - 1) & 63);
  for (int j = 0; j < n; j++) {
    const uint32_t c = canonical(text[(int64_t)j * stride]);
    const uint64_t *eqp = masks + (int64_t)find_slot(keys, c) * W;
    int hin = 1;
EDIT_UNROLL
    for (int w = 0; w < W; w++) {
      uint64_t eq = eqp[w];
      const uint64_t neg = hin < 0 ? 1ull : 0ull;
      const uint64_t xv = eq | mv[w];
      eq |= neg;
      const uint64_t xh = (((eq & pv[w]) + pv[w]) ^ pv[w]) | eq;
      uint64_t ph = mv[w] | ~(xh | pv[w]);
      uint64_t mh = pv[w] & xh;
      if (w == W - 1) score += (ph & top) ? 1 : (mh & top) ? -1 : 0;
      const int hout = (int)(ph >> 63) - (int)(mh >> 63);
      ph = (ph << 1) | (hin > 0 ? 1ull : 0ull);
      mh = (mh << 1) | neg;
      pv[w] = mh | ~(xv | ph);
      mv[w] = ph & xv;
      hin = hout;
    }
  }
  return score;
}

// m in 0..256.  m = 0: the distance is the length of the text.
EDIT_HD int32_t distance_any(const uint32_t *keys, const uint64_t *masks, int m, const uint32_t *text, int64_t stride, int n) {
  if (m == 0) return n;
  if (m <= 64) return distance<1>(keys, masks, m, text, stride, n);
  if (m <= 128) return distance<2>(keys, masks, m, text, stride, n);
  if (m <= 192) return distance<3>(keys, masks, m, text, stride, n);
  return distance<4>(keys, masks, m, text, stride, n);
}

}  // namespace edit_core
