// polysemous.cpp -- the renumbering of a sub-quantizer's 256 codewords so that the Hamming distance of two code bytes tracks
// the distance of their codewords (include/polysemous_ann.h: polysemous_optimize_codebook).  Host only: no device call.
//
// What it replaces: Faiss's PolysemousTraining::optimize_reproduce_distances (ReproduceDistancesObjective under a
// SimulatedAnnealingOptimizer), which index_factory turns on for every `PQ<M>` that does not end in `np`.  Faiss is not
// vendored in the reference: parity is UNPINNED.  Everything is fp64 in a fixed order; the draws come from mix64.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/polysemous_ann.h"
#include "abi_guard.h"
#define ABI_CATCH catch (...) { return abi_guard::caught(fail, IVF_ENOMEM, IVF_EINTERNAL); }

namespace {

thread_local std::string g_err;
int fail(int code, const std::string &m) {
  g_err = m;
  return code;
}

constexpr int KSUB = 256;
constexpr int64_t DEFAULT_ITERS = 500000;

// the 64-bit finaliser of sann_device.h (that header is device code; this file is compiled by the host compiler alone)
inline uint64_t mix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}
inline uint64_t draw(uint64_t seed, uint64_t step, uint64_t c) { return mix64(seed + 0x9E3779B97F4A7C15ull * (3 * step + c + 1)); }

inline double sq(double x) { return x * x; }
inline int ham(uint8_t a, uint8_t b) { return __builtin_popcount((unsigned)(a ^ b)); }

struct Objective {
  std::vector<double> t, w;  // [256][256]; the diagonal is never read
  bool flat = false;         // std == 0: nothing to optimise

  double cost(const uint8_t *p) const {
    double c = 0;
    for (int i = 0; i < KSUB; ++i)
      for (int j = 0; j < KSUB; ++j)
        if (i != j) c += w[(size_t)i * KSUB + j] * sq(t[(size_t)i * KSUB + j] - (double)ham(p[i], p[j]));
    return c;
  }
  // cost(p with the labels of i and j swapped) - cost(p): the (i, j) and (j, i) terms keep their Hamming distance
  double delta(const uint8_t *p, int i, int j) const {
    const double *ti = &t[(size_t)i * KSUB], *tj = &t[(size_t)j * KSUB], *wi = &w[(size_t)i * KSUB], *wj = &w[(size_t)j * KSUB];
    const uint8_t pi = p[i], pj = p[j];
    double acc = 0;
    for (int k = 0; k < KSUB; ++k) {
      if (k == i || k == j) continue;
      const double hi = (double)ham(pi, p[k]), hj = (double)ham(pj, p[k]);
      acc += wi[k] * (sq(ti[k] - hj) - sq(ti[k] - hi));
      acc += wj[k] * (sq(tj[k] - hi) - sq(tj[k] - hj));
    }
    return 2.0 * acc;
  }
};

void make_objective(int dsub, const float *cb, Objective &o) {
  std::vector<double> D((size_t)KSUB * KSUB, 0.0);
  for (int i = 0; i < KSUB; ++i)
    for (int j = 0; j < KSUB; ++j) {
      double s = 0;
      for (int c = 0; c < dsub; ++c) s += sq((double)cb[(size_t)i * dsub + c] - (double)cb[(size_t)j * dsub + c]);
      D[(size_t)i * KSUB + j] = s;
    }
  const double count = (double)KSUB * (KSUB - 1);
  double sum = 0;
  for (int i = 0; i < KSUB; ++i)
    for (int j = 0; j < KSUB; ++j)
      if (i != j) sum += D[(size_t)i * KSUB + j];
  const double mean = sum / count;
  double var = 0;
  for (int i = 0; i < KSUB; ++i)
    for (int j = 0; j < KSUB; ++j)
      if (i != j) var += sq(D[(size_t)i * KSUB + j] - mean);
  const double sd = std::sqrt(var / count);
  o.flat = !(sd > 0.0) || !std::isfinite(sd);
  o.t.assign((size_t)KSUB * KSUB, 4.0);
  o.w.assign((size_t)KSUB * KSUB, 0.0);
  const double ln2 = std::log(2.0), root2 = std::sqrt(2.0);
  for (size_t e = 0; e < o.t.size(); ++e) {
    if (!o.flat) o.t[e] = (D[e] - mean) / sd * root2 + 4.0;
    o.w[e] = std::exp(-ln2 * o.t[e]);
  }
}

}  // namespace

extern "C" {

const char *polysemous_last_error(void) { return g_err.c_str(); }

int polysemous_optimize_codebook(int32_t dsub, const float *codebook, int64_t iters, uint64_t seed, uint8_t *out_perm,
                                 double *cost_before, double *cost_after) try {
  if (!codebook || !out_perm || !cost_before || !cost_after) return fail(IVF_EINVAL, "null argument");
  if (dsub < 1 || dsub > 512) return fail(IVF_EINVAL, "dsub must be in 1..512");
  if (iters < 0) return fail(IVF_EINVAL, "iters must be 0 (500000 steps) or a number of steps");
  for (size_t e = 0; e < (size_t)KSUB * dsub; ++e)
    if (!std::isfinite(codebook[e])) return fail(IVF_EINVAL, "the codebook holds a value that is not finite");
  const int64_t steps = iters == 0 ? DEFAULT_ITERS : iters;
  Objective o;
  make_objective(dsub, codebook, o);
  uint8_t identity[KSUB], p[KSUB], best[KSUB];
  for (int j = 0; j < KSUB; ++j) identity[j] = p[j] = best[j] = (uint8_t)j;
  const double before = o.cost(identity);
  *cost_before = before;
  if (!o.flat) {
    const double decay = std::pow(0.9, 1.0 / 500.0);
    double temperature = 0.7, running = before, best_cost = before;
    for (int64_t s = 0; s < steps; ++s) {
      const int i = (int)(draw(seed, (uint64_t)s, 0) % KSUB);
      int j = (int)(draw(seed, (uint64_t)s, 1) % (KSUB - 1));
      if (j >= i) ++j;
      const double u = (double)(draw(seed, (uint64_t)s, 2) >> 11) * 0x1p-53;
      const double dl = o.delta(p, i, j);
      if (dl < 0 || u < temperature) {
        const uint8_t x = p[i];
        p[i] = p[j];
        p[j] = x;
        running += dl;
        if (running < best_cost) {
          best_cost = running;
          std::memcpy(best, p, KSUB);
        }
      }
      temperature *= decay;
    }
  }
  // the running cost carries the rounding of its deltas: the answer is judged by the formula in full
  double after = o.cost(best);
  if (!(after < before)) {
    std::memcpy(best, identity, KSUB);
    after = before;
  }
  std::memcpy(out_perm, best, KSUB);
  *cost_after = after;
  return IVF_OK;
} ABI_CATCH

}  // extern "C"
