// edit_host.cpp -- the host-only part of include/edit_ann.h: the error channel, the checks of caller data, the plain
// dynamic programme (edit_pair_distances_host) and the NearestNeighborResult codec with the editDistance arm.  No HIP call
// and no HIP header: g++ builds it, and tests/edit_host_check.cpp links it alone under the sanitizers.
// The wire format is Apache Thrift's TBinaryProtocol, restated from its published specification as in ann_codec.cpp.
#include <cstring>
#include <string>
#include <vector>

#include "edit_internal.h"

namespace edit_host {

namespace {
thread_local std::string g_err;
}

int fail(int code, const std::string &message) {
  g_err = message;
  return code;
}

int check_csr(const char *what, int64_t n, const int64_t *offsets, const float *chars, int64_t n_chars) {
  const std::string w(what);
  if (n < 0) return fail(EDIT_EINVAL, w + ": negative count");
  if (n == 0) return EDIT_OK;
  if (!offsets) return fail(EDIT_EINVAL, w + ": offsets is NULL");
  if (n_chars < 0) return fail(EDIT_EINVAL, w + ": negative n_chars");
  if (offsets[0] < 0) return fail(EDIT_EINVAL, w + ": offsets[0] is negative");
  for (int64_t i = 0; i < n; i++) {
    const int64_t a = offsets[i], b = offsets[i + 1];
    if (b < a) return fail(EDIT_EINVAL, w + ": offsets decrease at " + std::to_string(i + 1));
    if (b > n_chars) return fail(EDIT_EINVAL, w + ": offsets[" + std::to_string(i + 1) + "] = " + std::to_string(b) + " lies past the " + std::to_string(n_chars) + " elements of chars");
    if (b - a > EDIT_MAX_LENGTH) return fail(EDIT_ELIMIT, w + ": string " + std::to_string(i) + " has " + std::to_string(b - a) + " elements, the limit is " + std::to_string(EDIT_MAX_LENGTH));
  }
  if (offsets[n] > offsets[0] && !chars) return fail(EDIT_EINVAL, w + ": chars is NULL");
  return EDIT_OK;
}

// Metric.scala:189-220 bottom-up: cell (i, j) is the distance of the first i elements of a to the first j of b;
// (0, j) = j and (i, 0) = i (:197-198); equal elements take the diagonal (:206-207), unequal ones 1 + the least of insert
// (i, j - 1), delete (i - 1, j) and replace (i - 1, j - 1) (:211-215).  The memoised recursion visits a subset of these
// cells and gives each the same value.
int32_t plain_distance(const float *a, int la, const float *b, int lb) {
  int32_t prev[EDIT_MAX_LENGTH + 1], cur[EDIT_MAX_LENGTH + 1];
  for (int j = 0; j <= lb; j++) prev[j] = j;
  for (int i = 1; i <= la; i++) {
    cur[0] = i;
    const float ai = a[i - 1];
    for (int j = 1; j <= lb; j++) {
      if (ai == b[j - 1]) {
        cur[j] = prev[j - 1];
      } else {
        const int32_t insert = cur[j - 1], del = prev[j], replace = prev[j - 1];
        const int32_t least = insert < del ? insert : del;
        cur[j] = 1 + (least < replace ? least : replace);
      }
    }
    std::memcpy(prev, cur, sizeof(int32_t) * (size_t)(lb + 1));
  }
  return prev[lb];
}

namespace {

enum : uint8_t { T_STOP = 0, T_BOOL = 2, T_BYTE = 3, T_DOUBLE = 4, T_I16 = 6, T_I32 = 8, T_I64 = 10, T_STRING = 11, T_STRUCT = 12, T_MAP = 13, T_SET = 14, T_LIST = 15 };

// counts always, stores while there is room
struct W {
  uint8_t *p;
  int64_t cap, n = 0;
  W(uint8_t *buf, int64_t c) : p(buf), cap(buf && c > 0 ? c : 0) {}
  void u8(uint8_t v) { if (n < cap) p[n] = v; n++; }
  void i16(int16_t v) { u8((uint8_t)((uint16_t)v >> 8)); u8((uint8_t)v); }
  void i32(int32_t v) { for (int s = 24; s >= 0; s -= 8) u8((uint8_t)((uint32_t)v >> s)); }
  void i64(int64_t v) { for (int s = 56; s >= 0; s -= 8) u8((uint8_t)((uint64_t)v >> s)); }
  void field(uint8_t type, int16_t id) { u8(type); i16(id); }
};

struct R {
  const uint8_t *p;
  int64_t n, o = 0;
  bool bad = false;  // ran off the end, or met a value that cannot be skipped
  R(const uint8_t *buf, int64_t len) : p(buf), n(len) {}
  bool need(int64_t k) { if (bad || k < 0 || k > n - o) { bad = true; return false; } return true; }
  uint8_t u8() { if (!need(1)) return 0; return p[o++]; }
  int16_t i16() { if (!need(2)) return 0; const uint16_t v = (uint16_t)((p[o] << 8) | p[o + 1]); o += 2; return (int16_t)v; }
  int32_t i32() { if (!need(4)) return 0; uint32_t v = 0; for (int i = 0; i < 4; i++) v = (v << 8) | p[o + i]; o += 4; return (int32_t)v; }
  int64_t i64() { if (!need(8)) return 0; uint64_t v = 0; for (int i = 0; i < 8; i++) v = (v << 8) | p[o + i]; o += 8; return (int64_t)v; }
  void advance(int64_t k) { if (need(k)) o += k; }
  void skip(uint8_t type, int depth = 0) {
    if (depth > 64) { bad = true; return; }
    switch (type) {
      case T_BOOL: case T_BYTE: advance(1); return;
      case T_I16: advance(2); return;
      case T_I32: advance(4); return;
      case T_I64: case T_DOUBLE: advance(8); return;
      case T_STRING: { const int32_t len = i32(); advance(len); return; }
      case T_STRUCT:
        while (!bad) {
          const uint8_t t = u8();
          if (bad || t == T_STOP) return;
          i16();
          skip(t, depth + 1);
        }
        return;
      case T_MAP: {
        const uint8_t kt = u8(), vt = u8();
        const int32_t sz = i32();
        if (sz < 0) bad = true;
        for (int32_t i = 0; i < sz && !bad; i++) { skip(kt, depth + 1); skip(vt, depth + 1); }
        return;
      }
      case T_SET: case T_LIST: {
        const uint8_t et = u8();
        const int32_t sz = i32();
        if (sz < 0) bad = true;
        for (int32_t i = 0; i < sz && !bad; i++) skip(et, depth + 1);
        return;
      }
      default: bad = true;
    }
  }
};

// Reads the fields of a struct up to its stop byte; on_field(id, type) returns true when it consumed the value, false to
// have it skipped.  Errors travel in r.bad and in `format` (a message, set by the callbacks).
template <class F>
void read_struct(R &r, F on_field) {
  while (!r.bad) {
    const uint8_t t = r.u8();
    if (r.bad || t == T_STOP) return;
    const int16_t id = r.i16();
    if (r.bad) return;
    if (!on_field(id, t)) r.skip(t);
  }
}

}  // namespace
}  // namespace edit_host

using namespace edit_host;

extern "C" {

const char *edit_last_error(void) { return g_err.c_str(); }

int edit_pair_distances_host(int64_t n_pairs, const int64_t *a_offsets, const float *a_chars, int64_t n_a_chars, const int64_t *b_offsets,
                             const float *b_chars, int64_t n_b_chars, int32_t *out) try {
  if (int rc = check_csr("a", n_pairs, a_offsets, a_chars, n_a_chars)) return rc;
  if (int rc = check_csr("b", n_pairs, b_offsets, b_chars, n_b_chars)) return rc;
  if (n_pairs > 0 && !out) return fail(EDIT_EINVAL, "out is NULL");
  for (int64_t i = 0; i < n_pairs; i++)
    out[i] = plain_distance(a_chars + a_offsets[i], (int)(a_offsets[i + 1] - a_offsets[i]), b_chars + b_offsets[i],
                            (int)(b_offsets[i + 1] - b_offsets[i]));
  return EDIT_OK;
} EDIT_ABI_CATCH

int edit_wire_encode_neighbor_result(int32_t count, const int64_t *ids, const int32_t *distances, uint8_t *buf, int64_t cap,
                                     int64_t *len) try {
  if (count < 0 || (count > 0 && !ids)) return fail(EDIT_EINVAL, "bad neighbour arrays");
  W w(buf, cap);
  w.field(T_LIST, 1); w.u8(T_STRUCT); w.i32(count);  // 1: required list<NearestNeighbor> nearestNeighbors
  for (int32_t i = 0; i < count; i++) {
    w.field(T_STRING, 1); w.i32(8); w.i64(ids[i]);   // 1: required binary id (Injection.long2BigEndian)
    if (distances) {
      w.field(T_STRUCT, 2);                            // 2: optional Distance distance (union)
      w.field(T_STRUCT, 4);                            //    4: EditDistance editDistance
      w.field(T_I32, 1); w.i32(distances[i]);          //       1: required i32 distance
      w.u8(T_STOP);
      w.u8(T_STOP);
    }
    w.u8(T_STOP);
  }
  w.u8(T_STOP);
  if (len) *len = w.n;
  return w.n <= w.cap ? EDIT_OK : fail(EDIT_ESPACE, "output buffer too small: " + std::to_string(w.n) + " bytes needed");
} EDIT_ABI_CATCH

int edit_wire_decode_neighbor_result(const uint8_t *buf, int64_t n, int32_t cap, int64_t *ids, int32_t *distances, int32_t *arms,
                                     int32_t *count, int64_t *consumed) try {
  if (!buf || n < 0 || cap < 0) return fail(EDIT_EINVAL, "NULL buffer or negative size");
  R r(buf, n);
  const char *format = nullptr;
  bool seen = false;
  int32_t total = 0;
  read_struct(r, [&](int id, uint8_t t) -> bool {
    if (id != 1) return false;
    if (t != T_LIST) { format = "NearestNeighborResult: field 1 is not a list"; r.bad = true; return true; }
    const uint8_t et = r.u8();
    const int32_t sz = r.i32();
    if (r.bad) return true;
    if (et != T_STRUCT || sz < 0) { format = "NearestNeighborResult: not a list of structs"; r.bad = true; return true; }
    seen = true;
    total = sz;
    for (int32_t i = 0; i < sz && !r.bad; i++) {
      int64_t key = 0;
      int32_t dist = 0, arm = 0;
      bool have = false;
      read_struct(r, [&](int id2, uint8_t t2) -> bool {
        if (id2 == 1) {
          if (t2 != T_STRING) { format = "NearestNeighbor: id is not a binary"; r.bad = true; return true; }
          const int32_t len = r.i32();
          if (r.bad) return true;
          if (len != 8) { format = "NearestNeighbor: id is not an 8-byte long key"; r.bad = true; return true; }
          key = r.i64();
          have = !r.bad;
          return true;
        }
        if (id2 == 2 && t2 == T_STRUCT) {
          read_struct(r, [&](int id3, uint8_t t3) -> bool {
            if (id3 != 4 || t3 != T_STRUCT) return false;  // another arm: skipped, arm stays 0
            read_struct(r, [&](int id4, uint8_t t4) -> bool {
              if (id4 != 1 || t4 != T_I32) return false;
              dist = r.i32();
              arm = 4;
              return true;
            });
            return true;
          });
          return true;
        }
        return false;
      });
      if (r.bad) break;
      if (!have) { format = "NearestNeighbor: id is missing"; r.bad = true; break; }
      if (i < cap) {
        if (ids) ids[i] = key;
        if (distances) distances[i] = dist;
        if (arms) arms[i] = arm;
      }
    }
    return true;
  });
  if (r.bad) return fail(EDIT_EFORMAT, format ? format : "NearestNeighborResult: input ends inside a value or holds a malformed one");
  if (!seen) return fail(EDIT_EFORMAT, "NearestNeighborResult: nearestNeighbors is missing");
  if (count) *count = total;
  if (consumed) *consumed = r.o;
  if (total > cap && (ids || distances || arms)) return fail(EDIT_ESPACE, "more neighbours than the output arrays hold");
  return EDIT_OK;
} EDIT_ABI_CATCH

}  // extern "C"
