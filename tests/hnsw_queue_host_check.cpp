// hnsw_queue_host_check.cpp -- the one heap of the HNSW code (the-algorithm_amd/csrc/hnsw_queue.h: heap_add / heap_poll over a
// store and an order) against java.util.PriorityQueue written out below as the JDK writes it.  Random offer / poll sequences
// of up to 300 entries whose distances come from a pool of 12 values -- ties are the rule -- with both zeros, +inf, NaNs of
// non-canonical payload, negatives and a denormal.  After every operation the arrays must be equal entry for entry, bit for
// bit, for every instantiation: the plain HEntry array under both orders, a store split between two arrays after 1, 2, 3 and 7
// entries, and the KEntry array under the integer-key order, which must be the HEntry run under dist_key / key_dist.
// A stand-alone program: built with the address and undefined-behaviour sanitizers by tests/test_hnsw_queue_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "hnsw_queue.h"

namespace {

// ---- java.lang.Float.compare and java.util.PriorityQueue.offer / poll, restated on their own (not the header's) ----
int32_t java_float_to_int_bits(float f) {
  int32_t i;
  std::memcpy(&i, &f, 4);
  if ((i & 0x7f800000) == 0x7f800000 && (i & 0x007fffff) != 0) return 0x7fc00000;
  return i;
}
int java_float_compare(float f1, float f2) {
  if (f1 < f2) return -1;
  if (f1 > f2) return 1;
  const int32_t thisBits = java_float_to_int_bits(f1), anotherBits = java_float_to_int_bits(f2);
  return thisBits == anotherBits ? 0 : (thisBits < anotherBits ? -1 : 1);
}

constexpr int CAP = 300;

struct JavaPriorityQueue {
  HEntry queue[CAP];
  int size = 0;
  bool min_first;  // DistancedItemQueue: Float.compare(distance) or its reverse
  int compare(const HEntry &a, const HEntry &b) const {
    return min_first ? java_float_compare(a.dist, b.dist) : java_float_compare(b.dist, a.dist);
  }
  void offer(HEntry e) {
    const int i = size;
    size = i + 1;
    if (i == 0) queue[0] = e;
    else sift_up(i, e);
  }
  void sift_up(int k, HEntry x) {
    while (k > 0) {
      const int parent = (k - 1) >> 1;
      const HEntry e = queue[parent];
      if (compare(x, e) >= 0) break;
      queue[k] = e;
      k = parent;
    }
    queue[k] = x;
  }
  HEntry poll() {
    const int s = --size;
    const HEntry result = queue[0];
    const HEntry x = queue[s];
    if (s != 0) sift_down(0, x);
    return result;
  }
  void sift_down(int k, HEntry x) {
    const int half = size >> 1;
    while (k < half) {
      int child = (k << 1) + 1;
      HEntry c = queue[child];
      const int right = child + 1;
      if (right < size && compare(c, queue[right]) > 0) c = queue[child = right];
      if (compare(x, c) <= 0) break;
      queue[k] = c;
      k = child;
    }
    queue[k] = x;
  }
};

// a store split between two host arrays: entries [0, na) in a, the rest in b
template <class Entry>
struct SplitStore {
  Entry *a, *b;
  int na;
  Entry get(int i) const { return i < na ? a[i] : b[i - na]; }
  void set(int i, const Entry &e) const {
    if (i < na) a[i] = e;
    else b[i - na] = e;
  }
};

float from_bits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}
uint32_t bits_of(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}
const uint32_t POOL[12] = {
    0x00000000u,  // +0.0
    0x80000000u,  // -0.0
    0x7f800000u,  // +inf
    0x7fc12345u,  // NaN, payload
    0xffa00001u,  // NaN, sign set, signalling pattern
    0xbfc00000u,  // -1.5
    0xc0400000u,  // -3.0
    0x00000001u,  // the least denormal
    0x3e800000u,  // 0.25
    0x3f800000u,  // 1.0
    0x40200000u,  // 2.5
    0x40e00000u,  // 7.0
};

uint64_t rng_state;
uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

long failures = 0;
void expect(bool ok, const char *what, int seq, long op) {
  if (ok) return;
  if (failures++ < 20) std::printf("sequence %d, operation %ld: %s\n", seq, op, what);
}
bool same(const HEntry &a, const HEntry &b) { return bits_of(a.dist) == bits_of(b.dist) && a.node == b.node; }
bool same(const KEntry &k, const HEntry &h) { return k.key == dist_key(h.dist) && k.node == h.node; }

const int SPLITS[4] = {1, 2, 3, 7};

template <bool MINQ>
long run_sequence(int seq) {
  JavaPriorityQueue java;
  java.min_first = MINQ;
  HEntry plain[CAP];
  KEntry keyed[CAP];
  HEntry lo[4][8], hi[4][CAP];
  KEntry klo[8], khi[CAP];
  int n_plain = 0, n_keyed = 0, n_split[4] = {0, 0, 0, 0}, n_ksplit = 0;
  const SplitStore<KEntry> ksplit{klo, khi, 3};
  const long ops = 1400;  // (the first half offers three times in four: the queue reaches its 300 entries)
  long done = 0;
  for (long op = 0; op < ops || java.size > 0; ++op, ++done) {
    // grow towards the cap in the first half, drain in the second; past `ops` only polls, until the queue is empty
    const bool offer = op < ops && java.size < CAP && (java.size == 0 || rnd() % 100 < (op < ops / 2 ? 75u : 35u));
    if (offer) {
      const HEntry e{from_bits(POOL[rnd() % 12]), rnd() % 1000};
      java.offer(e);
      pq_add<MINQ>(plain, n_plain, e);
      heap_add<KeyOrder<MINQ>>(ArrayStore<KEntry>{keyed}, n_keyed, KEntry{dist_key(e.dist), e.node});
      for (int s = 0; s < 4; ++s) heap_add<DistOrder<MINQ>>(SplitStore<HEntry>{lo[s], hi[s], SPLITS[s]}, n_split[s], e);
      heap_add<KeyOrder<MINQ>>(ksplit, n_ksplit, KEntry{dist_key(e.dist), e.node});
    } else {
      const HEntry want = java.poll();
      expect(same(pq_poll<MINQ>(plain, n_plain), want), "poll of the plain HEntry array", seq, op);
      expect(same(heap_poll<KeyOrder<MINQ>>(ArrayStore<KEntry>{keyed}, n_keyed), want), "poll of the KEntry array", seq, op);
      for (int s = 0; s < 4; ++s)
        expect(same(heap_poll<DistOrder<MINQ>>(SplitStore<HEntry>{lo[s], hi[s], SPLITS[s]}, n_split[s]), want),
               "poll of a split HEntry store", seq, op);
      expect(same(heap_poll<KeyOrder<MINQ>>(ksplit, n_ksplit), want), "poll of the split KEntry store", seq, op);
    }
    const int n = java.size;
    expect(n_plain == n && n_keyed == n && n_ksplit == n, "sizes", seq, op);
    for (int s = 0; s < 4; ++s) expect(n_split[s] == n, "size of a split store", seq, op);
    for (int i = 0; i < n; ++i) {
      const HEntry &w = java.queue[i];
      expect(same(plain[i], w), "plain HEntry array", seq, op);
      expect(same(keyed[i], w), "KEntry array under dist_key", seq, op);
      const bool nan = w.dist != w.dist;  // key_dist gives the distance back, a NaN as the canonical one
      expect(bits_of(key_dist(keyed[i].key)) == (nan ? 0x7fc00000u : bits_of(w.dist)), "key_dist(dist_key(d))", seq, op);
      for (int s = 0; s < 4; ++s) expect(same(SplitStore<HEntry>{lo[s], hi[s], SPLITS[s]}.get(i), w), "split HEntry store", seq, op);
      expect(same(ksplit.get(i), w), "split KEntry store", seq, op);
    }
  }
  return done;
}

}  // namespace

int main() {
  // the key order is Float.compare's, pair by pair over the pool
  for (int i = 0; i < 12; ++i)
    for (int j = 0; j < 12; ++j) {
      const float a = from_bits(POOL[i]), b = from_bits(POOL[j]);
      const int want = java_float_compare(a, b);
      expect(float_compare(a, b) == want, "float_compare", i, j);
      expect((dist_key(a) < dist_key(b) ? -1 : dist_key(a) > dist_key(b) ? 1 : 0) == want, "dist_key order", i, j);
    }
  long operations = 0;
  int sequences = 0;
  for (int seed = 1; seed <= 50; ++seed) {
    rng_state = 0x9E3779B97F4A7C15ull * (uint64_t)seed;
    operations += run_sequence<true>(sequences++);
    operations += run_sequence<false>(sequences++);
  }
  std::printf("%s: %d sequences, %ld operations, %ld failures\n", failures ? "FAILED" : "ok", sequences, operations, failures);
  return failures ? 1 : 0;
}
