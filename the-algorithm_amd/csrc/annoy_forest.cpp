// annoy_forest.cpp -- the host side of include/annoy_ann.h: the preparation of rows, the forest builder (Annoy's two-means
// splits with counter-based draws), the loader that validates a flat forest, and the getters.  Pure host code, no HIP call;
// compiled with g++ -ffp-contract=off (the margin is an unfused multiply and add, the same function of the same bits as
// walk_kernel of annoy_ann.hip evaluates).  The layout and the semantics are stated in the header.
#include "annoy_forest.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <thread>

#include "../../include/annoy_ann.h"
#include "abi_guard.h"

namespace annoy_host {

std::string &error() {
  thread_local std::string e;
  return e;
}
int fail(int code, const std::string &m) {
  error() = m;
  return code;
}

bool prepare_rows(int metric, int d, int64_t n, const float *rows, uint16_t *out, int out_stride) {
  for (int64_t r = 0; r < n; ++r) {
    const float *x = rows + r * d;
    uint16_t *o = out + r * out_stride;
    // the sum of squares as store_rows_kernel adds it: lane l of 64 owns components l, l + 64, ...; then the xor tree
    double part[64];
    for (int l = 0; l < 64; ++l) part[l] = 0.0;
    for (int k = 0; k < d; ++k) {
      if (!std::isfinite(x[k])) return false;
      part[k & 63] += (double)x[k] * (double)x[k];
    }
    float norm = 1.0f;
    if (metric == IVF_METRIC_COSINE) {
      for (int s = 32; s; s >>= 1) {
        double t[64];
        for (int l = 0; l < 64; ++l) t[l] = part[l] + part[l ^ s];
        for (int l = 0; l < 64; ++l) part[l] = t[l];
      }
      norm = (float)std::sqrt(part[0]);
      if (!(norm > 0.0f)) norm = 1.0f;
    }
    for (int k = 0; k < d; ++k) o[k] = float_to_half(x[k] / norm);
    for (int k = d; k < out_stride; ++k) o[k] = 0;
  }
  return true;
}

}  // namespace annoy_host

namespace {

using annoy_host::fail;
#define ABI_CATCH catch (...) { return abi_guard::caught(fail, IVF_ENOMEM, IVF_EINTERNAL); }

inline uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
// draw number `j` of node `serial` of tree `tree`
inline uint64_t draw(uint64_t seed, uint64_t tree, uint64_t serial, uint64_t j) {
  uint64_t h = mix64(seed + 0x9e3779b97f4a7c15ull);
  h = mix64(h ^ tree);
  h = mix64(h ^ serial);
  return mix64(h ^ j);
}
constexpr uint64_t SIDE_DRAW = 1ull << 32;  // draw SIDE_DRAW + position: the side of a margin of exactly 0
constexpr int ATTEMPT_DRAWS = 256;          // draws of attempt a: a * 256 + (0, 1: the seeds; 2..201: the steps)
constexpr int STEPS = 200, REDRAWS = 3;

// what every entry refuses about the shape, before anything else
int check_shape(int32_t metric, int32_t d, int64_t n, int32_t n_trees, int32_t leaf_size) {
  if (metric == IVF_METRIC_INNER_PRODUCT)
    return fail(IVF_EINVAL, "InnerProduct is not supported by Annoy: the metric must be L2 or Cosine");
  if (metric != IVF_METRIC_L2 && metric != IVF_METRIC_COSINE) return fail(IVF_EINVAL, "unknown metric");
  if (d < 1 || d > ANNOY_MAX_D) return fail(IVF_EINVAL, "dimension must be in 1..1024");
  if (n < 1) return fail(IVF_EINVAL, "n must be positive");
  if (n >= (1ll << 31)) return fail(IVF_ELIMIT, "n must be below 2^31");
  if (n_trees < 1 || n_trees > ANNOY_MAX_TREES) return fail(IVF_EINVAL, "n_trees must be in 1..1024");
  if (leaf_size != 0 && (leaf_size < 2 || leaf_size > ANNOY_MAX_LEAF)) return fail(IVF_EINVAL, "leaf_size must be 0 or in 2..2048");
  if ((int64_t)n_trees * n >= (1ll << 31)) return fail(IVF_ELIMIT, "n_trees * n must be below 2^31");
  return IVF_OK;
}

struct Tree {
  std::vector<int32_t> nodes;      // [m][4], children and item ranges local to the tree
  std::vector<int32_t> split_of;   // per node: index into the tree's normals in the order computed, or -1
  std::vector<uint16_t> normals;   // [splits][d] in the order computed
  std::vector<float> offsets;
  std::vector<int32_t> perm;       // [n]
  bool ok = true;
};

struct Builder {
  int metric, d, stride, leaf_size;
  int64_t n;
  uint64_t seed;
  const float *rows;  // prepared, widened to fp32, [n][stride]

  // Annoy's two-means over perm[b, e); false if the centroids coincide.  normal: stride floats (fp16 values), offset fp32.
  bool two_means(const int32_t *it, int64_t cnt, int t, int64_t serial, int attempt, std::vector<double> &p, std::vector<double> &q,
                 float *normal, uint16_t *normal16, float *offset) const {
    const uint64_t base = (uint64_t)attempt * ATTEMPT_DRAWS;
    const int64_t i = (int64_t)(draw(seed, t, serial, base) % (uint64_t)cnt);
    int64_t j = (int64_t)(draw(seed, t, serial, base + 1) % (uint64_t)(cnt - 1));
    j += j >= i;
    const float *ri = rows + (int64_t)it[i] * stride, *rj = rows + (int64_t)it[j] * stride;
    for (int c = 0; c < d; ++c) {
      p[c] = ri[c];
      q[c] = rj[c];
    }
    double ic = 1, jc = 1;
    for (int l = 0; l < STEPS; ++l) {
      const float *r = rows + (int64_t)it[draw(seed, t, serial, base + 2 + l) % (uint64_t)cnt] * stride;
      double di = 0, dj = 0;
      for (int c = 0; c < d; ++c) {
        const double a = p[c] - r[c], b = q[c] - r[c];
        di += a * a;
        dj += b * b;
      }
      di *= ic;
      dj *= jc;
      if (di < dj) {
        for (int c = 0; c < d; ++c) p[c] = (p[c] * ic + r[c]) / (ic + 1);
        ic += 1;
      } else if (dj < di) {
        for (int c = 0; c < d; ++c) q[c] = (q[c] * jc + r[c]) / (jc + 1);
        jc += 1;
      }
    }
    double nn = 0;
    for (int c = 0; c < d; ++c) nn += (p[c] - q[c]) * (p[c] - q[c]);
    nn = std::sqrt(nn);
    if (!(nn > 0) || !std::isfinite(nn)) return false;
    bool any = false;
    for (int c = 0; c < d; ++c) {
      normal16[c] = annoy_host::float_to_half((float)((p[c] - q[c]) / nn));
      normal[c] = annoy_host::half_to_float(normal16[c]);
      any |= normal[c] != 0.0f;
    }
    for (int c = d; c < stride; ++c) normal[c] = 0.0f;
    if (!any) return false;
    double off = 0;
    if (metric == IVF_METRIC_L2) {
      for (int c = 0; c < d; ++c) off += (double)normal[c] * ((p[c] + q[c]) * 0.5);
      off = -off;
    }
    *offset = (float)off;
    return true;
  }

  void build_tree(int t, Tree &tr) const {
    tr.perm.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) tr.perm[(size_t)i] = (int32_t)i;
    struct Job {
      int64_t node, b, e;
    };
    std::vector<Job> stack;
    std::vector<double> p((size_t)d), q((size_t)d);
    std::vector<float> normal((size_t)stride);
    std::vector<uint16_t> normal16((size_t)d);
    std::vector<int32_t> left, right;
    std::vector<uint8_t> side;
    auto new_node = [&]() {
      tr.nodes.insert(tr.nodes.end(), 4, 0);
      tr.split_of.push_back(-1);
      return (int64_t)tr.split_of.size() - 1;
    };
    stack.push_back({new_node(), 0, n});
    while (!stack.empty()) {
      const Job jb = stack.back();
      stack.pop_back();
      const int64_t cnt = jb.e - jb.b;
      int32_t *it = tr.perm.data() + jb.b;
      if (cnt <= leaf_size) {
        int32_t *nd = &tr.nodes[(size_t)jb.node * 4];
        nd[0] = ANNOY_NODE_LEAF;
        nd[1] = (int32_t)jb.b;
        nd[2] = (int32_t)cnt;
        continue;
      }
      side.resize((size_t)cnt);
      bool good = false;
      float offset = 0.0f;
      for (int attempt = 0; attempt <= REDRAWS && !good; ++attempt) {
        if (!two_means(it, cnt, t, jb.node, attempt, p, q, normal.data(), normal16.data(), &offset)) continue;
        int64_t nr = 0;
        for (int64_t i = 0; i < cnt; ++i) {
          const float m = annoy_host::margin(normal.data(), rows + (int64_t)it[i] * stride, stride, offset, metric == IVF_METRIC_L2);
          uint8_t s;
          if (m > 0.0f) s = 1;
          else if (m < 0.0f) s = 0;
          else s = (uint8_t)(draw(seed, t, jb.node, SIDE_DRAW + (uint64_t)it[i]) & 1u);
          side[(size_t)i] = s;
          nr += s;
        }
        good = (double)std::max(nr, cnt - nr) <= 0.99 * (double)cnt;
      }
      int32_t flags = 0;
      if (!good) {  // the fallback split: alternately left and right
        flags = ANNOY_NODE_FALLBACK;
        for (int c = 0; c < d; ++c) normal16[c] = 0;
        offset = 0.0f;
        for (int64_t i = 0; i < cnt; ++i) side[(size_t)i] = (uint8_t)(i & 1);
      }
      left.clear();
      right.clear();
      for (int64_t i = 0; i < cnt; ++i) (side[(size_t)i] ? right : left).push_back(it[i]);
      std::copy(left.begin(), left.end(), it);
      std::copy(right.begin(), right.end(), it + left.size());
      const int64_t l = new_node(), r = new_node();
      int32_t *nd = &tr.nodes[(size_t)jb.node * 4];
      nd[0] = ANNOY_NODE_SPLIT;
      nd[1] = (int32_t)l;
      nd[2] = (int32_t)r;
      nd[3] = flags;
      tr.split_of[(size_t)jb.node] = (int32_t)tr.offsets.size();
      tr.offsets.push_back(offset);
      tr.normals.insert(tr.normals.end(), normal16.begin(), normal16.end());
      stack.push_back({r, jb.b + (int64_t)left.size(), jb.e});
      stack.push_back({l, jb.b, jb.b + (int64_t)left.size()});
    }
  }
};

int build(int32_t metric, int32_t d, int64_t n, const float *rows_fp32, int32_t n_trees, int32_t leaf_size, uint64_t seed,
          int32_t threads, annoy_forest_t **out) {
  if (int rc = check_shape(metric, d, n, n_trees, leaf_size)) return rc;
  if (threads < 0 || threads > ANNOY_MAX_THREADS) return fail(IVF_EINVAL, "threads must be in 0..16");
  if (!rows_fp32 || !out) return fail(IVF_EINVAL, "null argument");
  if (threads == 0) threads = std::min<int32_t>(ANNOY_MAX_THREADS, n_trees);
  threads = std::min(threads, n_trees);
  const int stride = (d + 7) / 8 * 8;
  std::vector<float> rows((size_t)n * stride);
  {
    std::vector<uint16_t> h((size_t)n * stride);
    if (!annoy_host::prepare_rows(metric, d, n, rows_fp32, h.data(), stride)) return fail(IVF_EINVAL, "a row component is not finite");
    for (size_t i = 0; i < h.size(); ++i) rows[i] = annoy_host::half_to_float(h[i]);
  }
  Builder b{metric, d, stride, leaf_size ? leaf_size : d + 2, n, seed, rows.data()};
  std::vector<Tree> trees((size_t)n_trees);
  auto work = [&](int first) {
    for (int t = first; t < n_trees; t += threads) {
      try {
        b.build_tree(t, trees[(size_t)t]);
      } catch (...) {
        trees[(size_t)t].ok = false;
      }
    }
  };
  if (threads == 1) {
    work(0);
  } else {
    std::vector<std::thread> pool;
    for (int i = 0; i < threads; ++i) pool.emplace_back(work, i);
    for (auto &th : pool) th.join();
  }
  int64_t n_nodes = 0, n_splits = 0;
  for (const Tree &tr : trees) {
    if (!tr.ok) return fail(IVF_ENOMEM, "out of host memory");
    n_nodes += (int64_t)tr.split_of.size();
    n_splits += (int64_t)tr.offsets.size();
  }
  if (n_nodes >= (1ll << 31)) return fail(IVF_ELIMIT, "the forest has 2^31 nodes or more");
  std::unique_ptr<annoy_forest> f(new annoy_forest);
  f->metric = metric;
  f->d = d;
  f->stride = stride;
  f->n_trees = n_trees;
  f->leaf_size = b.leaf_size;
  f->n = n;
  f->nodes.reserve((size_t)n_nodes * 4);
  f->normals.reserve((size_t)n_splits * d);
  f->offsets.reserve((size_t)n_splits);
  f->items.reserve((size_t)n_trees * n);
  for (int t = 0; t < n_trees; ++t) {
    Tree &tr = trees[(size_t)t];
    const int32_t node0 = (int32_t)f->n_nodes(), item0 = (int32_t)((int64_t)t * n);
    f->roots.push_back(node0);
    for (size_t v = 0; v < tr.split_of.size(); ++v) {
      const int32_t *nd = &tr.nodes[v * 4];
      if (nd[0] == ANNOY_NODE_LEAF) {
        f->nodes.insert(f->nodes.end(), {nd[0], nd[1] + item0, nd[2], nd[3]});
        f->max_leaf = std::max(f->max_leaf, nd[2]);
      } else {
        f->nodes.insert(f->nodes.end(), {nd[0], nd[1] + node0, nd[2] + node0, nd[3]});
        const size_t s = (size_t)tr.split_of[v];
        f->offsets.push_back(tr.offsets[s]);
        f->normals.insert(f->normals.end(), tr.normals.begin() + s * d, tr.normals.begin() + (s + 1) * d);
      }
    }
    f->items.insert(f->items.end(), tr.perm.begin(), tr.perm.end());
    tr = Tree();
  }
  *out = f.release();
  return IVF_OK;
}

int load(int32_t metric, int32_t d, int64_t n, int32_t n_trees, int32_t leaf_size, int64_t n_nodes, const int32_t *nodes,
         int64_t n_splits, const uint16_t *normals, const float *offsets, const int32_t *roots, int64_t n_items,
         const int32_t *items, annoy_forest_t **out) {
  if (n < 0 || n_nodes < 0 || n_splits < 0 || n_items < 0) return fail(IVF_EINVAL, "a count is negative");
  if (int rc = check_shape(metric, d, n, n_trees, leaf_size)) return rc;
  if (!nodes || !roots || !items || !out) return fail(IVF_EINVAL, "null argument");
  if (n_nodes >= (1ll << 31)) return fail(IVF_ELIMIT, "the forest has 2^31 nodes or more");
  if (n_nodes < n_trees) return fail(IVF_EINVAL, "fewer nodes than trees");
  if (n_items != (int64_t)n_trees * n) return fail(IVF_EINVAL, "n_items must be n_trees * n");
  if (n_splits > n_nodes || (n_splits > 0 && (!normals || !offsets))) return fail(IVF_EINVAL, "splits without normals or offsets");
  const int32_t leaf = leaf_size ? leaf_size : d + 2;
  // the nodes one by one
  int64_t splits = 0;
  int32_t max_leaf = 0;
  for (int64_t v = 0; v < n_nodes; ++v) {
    const int32_t *nd = nodes + v * 4;
    const std::string at = "node " + std::to_string(v) + ": ";
    if (nd[3] & ~ANNOY_NODE_FALLBACK) return fail(IVF_EINVAL, at + "unknown flag bits");
    if (nd[0] == ANNOY_NODE_SPLIT) {
      if (nd[1] < 0 || nd[1] >= n_nodes || nd[2] < 0 || nd[2] >= n_nodes) return fail(IVF_EINVAL, at + "a child is out of range");
      ++splits;
    } else if (nd[0] == ANNOY_NODE_LEAF) {
      if (nd[3]) return fail(IVF_EINVAL, at + "a leaf carries a split's flag");
      if (nd[2] < 1 || nd[2] > leaf) return fail(IVF_EINVAL, at + "a leaf holds " + std::to_string(nd[2]) + " items, outside 1.." + std::to_string(leaf));
      if (nd[1] < 0 || (int64_t)nd[1] + nd[2] > n_items) return fail(IVF_EINVAL, at + "the item range is outside the item array");
      max_leaf = std::max(max_leaf, nd[2]);
    } else {
      return fail(IVF_EINVAL, at + "unknown kind");
    }
  }
  if (splits != n_splits) return fail(IVF_EINVAL, "n_splits is not the number of split nodes");
  for (int64_t s = 0; s < n_splits; ++s) {
    if (!std::isfinite(offsets[s])) return fail(IVF_EINVAL, "an offset is not finite");
    if (metric == IVF_METRIC_COSINE && offsets[s] != 0.0f) return fail(IVF_EINVAL, "a Cosine split has an offset");
  }
  for (int64_t i = 0; i < n_splits * d; ++i)
    if ((normals[i] & 0x7c00u) == 0x7c00u) return fail(IVF_EINVAL, "a normal component is not finite");
  for (int64_t i = 0; i < n_items; ++i)
    if (items[i] < 0 || items[i] >= n) return fail(IVF_EINVAL, "an item is outside 0..n-1");
  // every tree a tree, every position once per tree
  std::vector<uint8_t> reached((size_t)n_nodes, 0);
  std::vector<int32_t> seen((size_t)n, -1);
  std::vector<int32_t> stack;
  for (int32_t t = 0; t < n_trees; ++t) {
    if (roots[t] < 0 || roots[t] >= n_nodes) return fail(IVF_EINVAL, "a root is out of range");
    int64_t got = 0;
    stack.assign(1, roots[t]);
    while (!stack.empty()) {
      const int32_t v = stack.back();
      stack.pop_back();
      if (reached[(size_t)v]) return fail(IVF_EINVAL, "node " + std::to_string(v) + " is reached twice: a cycle or a shared child");
      reached[(size_t)v] = 1;
      const int32_t *nd = nodes + (int64_t)v * 4;
      if (nd[0] == ANNOY_NODE_SPLIT) {
        stack.push_back(nd[2]);
        stack.push_back(nd[1]);
      } else {
        for (int32_t i = 0; i < nd[2]; ++i) {
          const int32_t x = items[(int64_t)nd[1] + i];
          if (seen[(size_t)x] == t) return fail(IVF_EINVAL, "item " + std::to_string(x) + " is twice in tree " + std::to_string(t));
          seen[(size_t)x] = t;
        }
        got += nd[2];
      }
    }
    if (got != n) return fail(IVF_EINVAL, "tree " + std::to_string(t) + " holds " + std::to_string(got) + " of " + std::to_string(n) + " items");
  }
  for (int64_t v = 0; v < n_nodes; ++v)
    if (!reached[(size_t)v]) return fail(IVF_EINVAL, "node " + std::to_string(v) + " is reached from no root");
  std::unique_ptr<annoy_forest> f(new annoy_forest);
  f->metric = metric;
  f->d = d;
  f->stride = (d + 7) / 8 * 8;
  f->n_trees = n_trees;
  f->leaf_size = leaf;
  f->max_leaf = max_leaf;
  f->n = n;
  f->nodes.assign(nodes, nodes + n_nodes * 4);
  if (n_splits) {
    f->normals.assign(normals, normals + n_splits * d);
    f->offsets.assign(offsets, offsets + n_splits);
  }
  f->roots.assign(roots, roots + n_trees);
  f->items.assign(items, items + n_items);
  *out = f.release();
  return IVF_OK;
}

template <class T>
int get(const std::vector<T> &v, T *out) {
  if (v.empty()) return IVF_OK;
  if (!out) return fail(IVF_EINVAL, "null argument");
  std::copy(v.begin(), v.end(), out);
  return IVF_OK;
}

}  // namespace

extern "C" {

const char *annoy_last_error(void) { return annoy_host::error().c_str(); }

int annoy_prepare_rows(int32_t metric, int32_t d, int64_t n, const float *rows_fp32, uint16_t *out) try {
  if (int rc = check_shape(metric, d, n > 0 ? 1 : n, 1, 0)) return rc;
  if (!rows_fp32 || !out) return fail(IVF_EINVAL, "null argument");
  if (!annoy_host::prepare_rows(metric, d, n, rows_fp32, out, d)) return fail(IVF_EINVAL, "a row component is not finite");
  return IVF_OK;
} ABI_CATCH

int annoy_forest_build(int32_t metric, int32_t d, int64_t n, const float *rows_fp32, int32_t n_trees, int32_t leaf_size,
                       uint64_t seed, int32_t threads, annoy_forest_t **out) try {
  return build(metric, d, n, rows_fp32, n_trees, leaf_size, seed, threads, out);
} ABI_CATCH

int annoy_forest_load(int32_t metric, int32_t d, int64_t n, int32_t n_trees, int32_t leaf_size, int64_t n_nodes,
                      const int32_t *nodes, int64_t n_splits, const uint16_t *normals, const float *offsets,
                      const int32_t *roots, int64_t n_items, const int32_t *items, annoy_forest_t **out) try {
  return load(metric, d, n, n_trees, leaf_size, n_nodes, nodes, n_splits, normals, offsets, roots, n_items, items, out);
} ABI_CATCH

int annoy_forest_info(const annoy_forest_t *f, int32_t *metric, int32_t *d, int64_t *n, int32_t *n_trees, int32_t *leaf_size,
                      int64_t *n_nodes, int64_t *n_splits, int64_t *n_items) try {
  if (!f) return fail(IVF_EINVAL, "null forest");
  if (metric) *metric = f->metric;
  if (d) *d = f->d;
  if (n) *n = f->n;
  if (n_trees) *n_trees = f->n_trees;
  if (leaf_size) *leaf_size = f->leaf_size;
  if (n_nodes) *n_nodes = f->n_nodes();
  if (n_splits) *n_splits = f->n_splits();
  if (n_items) *n_items = (int64_t)f->items.size();
  return IVF_OK;
} ABI_CATCH

int annoy_forest_get_nodes(const annoy_forest_t *f, int32_t *out) try { return f ? get(f->nodes, out) : fail(IVF_EINVAL, "null forest"); } ABI_CATCH
int annoy_forest_get_normals(const annoy_forest_t *f, uint16_t *out) try { return f ? get(f->normals, out) : fail(IVF_EINVAL, "null forest"); } ABI_CATCH
int annoy_forest_get_offsets(const annoy_forest_t *f, float *out) try { return f ? get(f->offsets, out) : fail(IVF_EINVAL, "null forest"); } ABI_CATCH
int annoy_forest_get_roots(const annoy_forest_t *f, int32_t *out) try { return f ? get(f->roots, out) : fail(IVF_EINVAL, "null forest"); } ABI_CATCH
int annoy_forest_get_items(const annoy_forest_t *f, int32_t *out) try { return f ? get(f->items, out) : fail(IVF_EINVAL, "null forest"); } ABI_CATCH

int annoy_forest_destroy(annoy_forest_t *f) try {
  delete f;
  return IVF_OK;
} ABI_CATCH

}  // extern "C"
