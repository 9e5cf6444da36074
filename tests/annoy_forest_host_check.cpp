// annoy_forest_host_check.cpp -- the host side of include/annoy_ann.h (the-algorithm_amd/csrc/annoy_forest.cpp) as a
// stand-alone program for the address and undefined-behaviour sanitizers: builds small forests, round-trips them through
// annoy_forest_load, and feeds the loader malformed ones.  No device, no HIP.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/annoy_ann.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
      ++failures;                                                    \
    }                                                                \
  } while (0)

uint64_t state = 12345;
float rnd() {
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return (float)((state >> 40) & 0xffff) / 65536.0f - 0.5f;
}

struct Flat {
  int32_t metric, d, n_trees, leaf;
  int64_t n, n_nodes, n_splits, n_items;
  std::vector<int32_t> nodes, roots, items;
  std::vector<uint16_t> normals;
  std::vector<float> offsets;
};

Flat flat_of(const annoy_forest_t *f) {
  Flat x;
  CHECK(annoy_forest_info(f, &x.metric, &x.d, &x.n, &x.n_trees, &x.leaf, &x.n_nodes, &x.n_splits, &x.n_items) == IVF_OK);
  x.nodes.resize((size_t)x.n_nodes * 4);
  x.roots.resize((size_t)x.n_trees);
  x.items.resize((size_t)x.n_items);
  x.normals.resize((size_t)x.n_splits * x.d);
  x.offsets.resize((size_t)x.n_splits);
  CHECK(annoy_forest_get_nodes(f, x.nodes.data()) == IVF_OK);
  CHECK(annoy_forest_get_roots(f, x.roots.data()) == IVF_OK);
  CHECK(annoy_forest_get_items(f, x.items.data()) == IVF_OK);
  CHECK(annoy_forest_get_normals(f, x.normals.data()) == IVF_OK);
  CHECK(annoy_forest_get_offsets(f, x.offsets.data()) == IVF_OK);
  return x;
}

int load(const Flat &x, annoy_forest_t **out) {
  return annoy_forest_load(x.metric, x.d, x.n, x.n_trees, x.leaf, x.n_nodes, x.nodes.data(), x.n_splits, x.normals.data(),
                           x.offsets.data(), x.roots.data(), x.n_items, x.items.data(), out);
}

void refused(const Flat &x, int code, const char *what) {
  annoy_forest_t *f = nullptr;
  const int rc = load(x, &f);
  if (rc != code || f != nullptr || !annoy_last_error()[0]) {
    std::printf("FAILED: %s: status %d, wanted %d\n", what, rc, code);
    ++failures;
  }
  if (f) annoy_forest_destroy(f);
}

int first_of(const Flat &x, int kind, int from = 0) {
  for (int64_t v = from; v < x.n_nodes; ++v)
    if (x.nodes[(size_t)v * 4] == kind) return (int)v;
  return -1;
}

}  // namespace

int main() {
  int forests = 0;
  const int dims[] = {1, 3, 8, 17, 64, 130};
  for (int metric : {IVF_METRIC_L2, IVF_METRIC_COSINE})
    for (int d : dims)
      for (int leaf : {2, 0, 9})
        for (int n : {1, 2, 37, 300}) {
          std::vector<float> rows((size_t)n * d);
          for (auto &v : rows) v = rnd();
          if (n == 37)  // a run of identical rows: fallback splits
            for (int r = 1; r < 20; ++r) std::memcpy(&rows[(size_t)r * d], &rows[0], (size_t)d * sizeof(float));
          annoy_forest_t *f = nullptr, *g = nullptr, *h = nullptr;
          CHECK(annoy_forest_build(metric, d, n, rows.data(), 3, leaf, 7, 1, &f) == IVF_OK);
          CHECK(annoy_forest_build(metric, d, n, rows.data(), 3, leaf, 7, 3, &g) == IVF_OK);
          if (!f || !g) return 1;
          Flat a = flat_of(f), b = flat_of(g);
          CHECK(a.nodes == b.nodes && a.items == b.items && a.normals == b.normals && a.roots == b.roots);
          CHECK(a.offsets.size() == b.offsets.size() &&
                (a.offsets.empty() || !std::memcmp(a.offsets.data(), b.offsets.data(), a.offsets.size() * sizeof(float))));
          CHECK(load(a, &h) == IVF_OK);
          if (h) {
            Flat c = flat_of(h);
            CHECK(c.nodes == a.nodes && c.items == a.items && c.normals == a.normals && c.roots == a.roots && c.leaf == a.leaf);
          }
          // the refusals
          if (n == 300) {
            const int s = first_of(a, ANNOY_NODE_SPLIT), l = first_of(a, ANNOY_NODE_LEAF);
            Flat x = a;
            x.nodes[(size_t)s * 4 + 1] = (int32_t)a.n_nodes;
            refused(x, IVF_EINVAL, "a child out of range");
            x = a;
            x.nodes[(size_t)s * 4 + 2] = -1;
            refused(x, IVF_EINVAL, "a negative child");
            const int c = first_of(a, ANNOY_NODE_SPLIT, s + 1);
            if (c >= 0) {  // a later split points back at the first: its subtree is entered twice
              x = a;
              x.nodes[(size_t)c * 4 + 1] = s;
              refused(x, IVF_EINVAL, "a cycle");
            }
            x = a;
            x.nodes[(size_t)s * 4 + 2] = x.nodes[(size_t)s * 4 + 1];
            refused(x, IVF_EINVAL, "a shared child");
            x = a;
            x.items[(size_t)a.nodes[(size_t)l * 4 + 1]] = x.items[(size_t)a.nodes[(size_t)l * 4 + 1] + 1];
            refused(x, IVF_EINVAL, "an item twice, another missing");
            x = a;
            x.items[0] = (int32_t)a.n;
            refused(x, IVF_EINVAL, "an item out of range");
            x = a;
            x.nodes[(size_t)l * 4 + 2] = a.leaf + 1;
            refused(x, IVF_EINVAL, "an oversized leaf");
            x = a;
            x.nodes[(size_t)l * 4 + 1] = (int32_t)a.n_items;
            refused(x, IVF_EINVAL, "an item range outside the array");
            x = a;
            x.nodes[(size_t)l * 4] = 5;
            refused(x, IVF_EINVAL, "an unknown kind");
            x = a;
            x.nodes[(size_t)s * 4 + 3] = 6;
            refused(x, IVF_EINVAL, "unknown flags");
            x = a;
            x.roots[0] = (int32_t)a.n_nodes;
            refused(x, IVF_EINVAL, "a root out of range");
            x = a;
            x.normals[0] = 0x7c00;
            refused(x, IVF_EINVAL, "an infinite normal");
            x = a;
            x.n_nodes = -1;
            refused(x, IVF_EINVAL, "a negative node count");
            x = a;
            x.n_items = -1;
            refused(x, IVF_EINVAL, "a negative item count");
            x = a;
            x.n = 1ll << 31;
            refused(x, IVF_ELIMIT, "2^31 items");
            x = a;
            x.metric = IVF_METRIC_INNER_PRODUCT;
            refused(x, IVF_EINVAL, "InnerProduct");
            x = a;
            x.n_splits -= 1;
            refused(x, IVF_EINVAL, "a wrong split count");
          }
          annoy_forest_destroy(f);
          annoy_forest_destroy(g);
          annoy_forest_destroy(h);
          ++forests;
        }
  std::printf("ok: %d forests, %d failures\n", forests, failures);
  return failures ? 1 : 0;
}
