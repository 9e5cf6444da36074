// annoy_forest.h -- the one flat host form of an Annoy forest (include/annoy_ann.h), shared by annoy_forest.cpp (builder,
// loader, getters: host only, g++), annoy_ann.hip (the index uploads it) and tests/annoy_forest_host_check.cpp.  No HIP here.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

struct annoy_forest {
  int32_t metric = 0, d = 0, stride = 0, n_trees = 0, leaf_size = 0, max_leaf = 0;
  int64_t n = 0;
  std::vector<int32_t> nodes;     // [n_nodes][4]: kind, a, b, flags
  std::vector<uint16_t> normals;  // [n_splits][d]
  std::vector<float> offsets;     // [n_splits]
  std::vector<int32_t> roots;     // [n_trees]
  std::vector<int32_t> items;     // [n_trees * n]
  int64_t n_nodes() const { return (int64_t)(nodes.size() / 4); }
  int64_t n_splits() const { return (int64_t)offsets.size(); }
};

namespace annoy_host {

// the message behind annoy_last_error(): one per thread, written by both translation units
std::string &error();
int fail(int code, const std::string &m);

inline float half_to_float(uint16_t h) {
  const uint32_t s = (uint32_t)(h & 0x8000u) << 16;
  uint32_t e = (h >> 10) & 31u, m = h & 1023u, u;
  if (e == 0) {
    if (m == 0) {
      u = s;
    } else {  // subnormal: renormalise
      int sh = 0;
      while (!(m & 1024u)) {
        m <<= 1;
        ++sh;
      }
      u = s | ((uint32_t)(113 - sh) << 23) | ((m & 1023u) << 13);
    }
  } else if (e == 31) {
    u = s | 0x7f800000u | (m << 13);
  } else {
    u = s | ((e + 112u) << 23) | (m << 13);
  }
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// round to nearest even, as the device's conversion
inline uint16_t float_to_half(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  const uint16_t s = (uint16_t)((u >> 16) & 0x8000u);
  u &= 0x7fffffffu;
  if (u >= 0x7f800000u) return (uint16_t)(s | 0x7c00u | (u > 0x7f800000u ? 0x200u : 0u));
  if (u >= 0x477ff000u) return (uint16_t)(s | 0x7c00u);  // rounds to infinity (65520 and above)
  if (u < 0x38800000u) {                                 // below the smallest normal half: a subnormal or zero
    if (u < 0x33000000u) return s;                       // below 2^-25: zero (2^-25 itself ties to even, zero)
    const int e = (int)(u >> 23);
    const uint32_t m = (u & 0x7fffffu) | 0x800000u;
    const int shift = 126 - e;  // 14..24: m * 2^(e - 150) in units of 2^-24
    const uint32_t q = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    return (uint16_t)(s | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u)));
  }
  const uint32_t v = u - 0x38000000u;  // exponent rebased, 23-bit mantissa
  const uint32_t q = v >> 13, rem = v & 0x1fffu;
  return (uint16_t)(s | (q + ((rem > 0x1000u || (rem == 0x1000u && (q & 1u))) ? 1u : 0u)));
}

// The margin of include/annoy_ann.h over rows already widened to fp32 and padded to `stride` (a multiple of 8, <= 1024): the
// host's emulation of the order that row_score.h states for the device (pieces l and l + 64 per lane, components 0..7, the
// xor tree).  Compiled with -ffp-contract=off: a multiply, then an add.
inline float margin(const float *normal, const float *q, int stride, float offset, bool l2) {
  float acc[64];
  for (int l = 0; l < 64; ++l) acc[l] = 0.0f;
  const int pieces = stride >> 3;
  for (int p = 0; p < pieces; ++p) {
    float a = acc[p & 63];
    for (int e = 0; e < 8; ++e) {
      const float prod = normal[p * 8 + e] * q[p * 8 + e];
      a = a + prod;
    }
    acc[p & 63] = a;
  }
  for (int o = 32; o; o >>= 1) {
    float t[64];
    for (int l = 0; l < 64; ++l) t[l] = acc[l] + acc[l ^ o];
    for (int l = 0; l < 64; ++l) acc[l] = t[l];
  }
  return l2 ? acc[0] + offset : acc[0];
}

// rows fp32 [n][d] -> fp16 bits [n][out_stride] (out_stride >= d; the padding is zeroed); false if a component is not finite
bool prepare_rows(int metric, int d, int64_t n, const float *rows, uint16_t *out, int out_stride);

}  // namespace annoy_host
