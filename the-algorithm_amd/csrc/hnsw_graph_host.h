// hnsw_graph_host.h -- the one host form of an HNSW graph: the device layout itself (hnsw_walk.h: SearchArgs) plus one
// "the reference's map holds the key HnswNode(level, item)" flag per row of storage.  A loaded graph is laid out into it, the
// host builder's result is (hnsw_host_builder.h), an export is emitted from it.  Pure C++: tests/hnsw_graph_host_check.cpp
// runs it under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace hnsw_graph {

struct FlatGraph {
  int64_t n = 0, entry = -1;
  int m = 0, m0 = 0, max_level = 0;
  std::vector<uint32_t> adj0;               // [n][m0 + 1]: count, neighbours
  std::vector<int32_t> upper_slot = {-1};   // [max(n, 1)]: row group of a node with storage above level 0, or -1
  std::vector<int32_t> upper_base = {0};    // [slots + 1]: first row of the slot; its rows are levels 1..top
  std::vector<uint32_t> upper_adj;          // [rows][m + 1]
  std::vector<uint8_t> has0, has_up;        // [n], [rows]: the key exists (a key may hold an empty list)

  // n rows of no keys and empty lists, with storage for levels 0..tops[i] of item i
  void init(int64_t n_, int max_m, const std::vector<int32_t> &tops) {
    n = n_;
    m = max_m;
    m0 = 2 * max_m;
    adj0.assign((size_t)n * (m0 + 1), 0);
    has0.assign((size_t)n, 0);
    upper_slot.assign((size_t)std::max<int64_t>(n, 1), -1);
    upper_base.assign(1, 0);
    for (int64_t i = 0; i < n; ++i)
      if (tops[(size_t)i] > 0) {
        upper_slot[(size_t)i] = (int32_t)upper_base.size() - 1;
        upper_base.push_back(upper_base.back() + tops[(size_t)i]);
      }
    upper_adj.assign((size_t)upper_base.back() * (m + 1), 0);
    has_up.assign((size_t)upper_base.back(), 0);
  }
  int64_t slots() const { return (int64_t)upper_base.size() - 1; }
  int64_t upper_row(int level, int64_t item) const { return upper_base[(size_t)upper_slot[(size_t)item]] + level - 1; }
  uint32_t *row(int level, int64_t item) {
    return level == 0 ? &adj0[(size_t)item * (m0 + 1)] : &upper_adj[(size_t)upper_row(level, item) * (m + 1)];
  }
  uint8_t &has(int level, int64_t item) { return level == 0 ? has0[(size_t)item] : has_up[(size_t)upper_row(level, item)]; }
};

// A graph given as entries: entry e is HnswNode(entry_level[e], entry_item[e]) with the neighbours
// entry_neighbours[entry_offsets[e] .. entry_offsets[e + 1]) (include/hnsw_ann.h: hnsw_index_build).  The caller has checked
// entry_point < n and 0 <= max_level.  Returns what is wrong with the entries, or NULL.
inline const char *from_entries(int64_t n, int max_m, int64_t entry_point, int max_level, int64_t n_entries,
                                const int32_t *entry_level, const int64_t *entry_item, const int64_t *entry_offsets,
                                const int64_t *entry_neighbours, FlatGraph &g) {
  std::vector<int32_t> tops((size_t)n, 0);
  for (int64_t e = 0; e < n_entries; ++e) {
    if (entry_level[e] < 0 || entry_level[e] > max_level || entry_item[e] < 0 || entry_item[e] >= n) return "graph entry out of range";
    tops[(size_t)entry_item[e]] = std::max(tops[(size_t)entry_item[e]], entry_level[e]);
  }
  // Rows also for every layer a node can be REACHED on without a key of its own there -- the entry point on layers up to
  // maxLevel, a neighbour on its list's layer: empty rows, which searches read as the absent list they are, and which an
  // append (whose walks read and whose back links write the rows of every node they reach) needs to exist.
  if (entry_point >= 0) tops[(size_t)entry_point] = std::max(tops[(size_t)entry_point], max_level);
  for (int64_t e = 0; e < n_entries && entry_neighbours; ++e) {
    if (entry_offsets[e + 1] < entry_offsets[e] || entry_offsets[e + 1] - entry_offsets[e] > 2 * (int64_t)max_m) continue;  // (refused below)
    for (int64_t j = entry_offsets[e]; j < entry_offsets[e + 1]; ++j)
      if (entry_neighbours[j] >= 0 && entry_neighbours[j] < n)
        tops[(size_t)entry_neighbours[j]] = std::max(tops[(size_t)entry_neighbours[j]], entry_level[e]);
  }
  g.init(n, max_m, tops);
  g.entry = entry_point < 0 ? -1 : entry_point;
  g.max_level = max_level;
  for (int64_t e = 0; e < n_entries; ++e) {
    const int level = entry_level[e];
    const int64_t b = entry_offsets[e], en = entry_offsets[e + 1];
    if (en < b || en - b > (level == 0 ? g.m0 : g.m)) return "neighbour list longer than the level allows";
    uint32_t *row = g.row(level, entry_item[e]);
    for (int64_t j = b; j < en; ++j) {
      if (!entry_neighbours || entry_neighbours[j] < 0 || entry_neighbours[j] >= n) return "neighbour out of range";
      row[1 + (j - b)] = (uint32_t)entry_neighbours[j];
    }
    row[0] = (uint32_t)(en - b);  // (a key given twice: the later list, as a map's put)
    g.has(level, entry_item[e]) = 1;  // a key given with an empty list exists
  }
  return nullptr;
}

// The export (hnsw_index_graph_size, hnsw_index_graph): an entry exists where its flag is set or its list is not empty (a back
// link made the key).  Order: level 0 by item ascending, then level 1, 2, ..., each by slot ascending.  `emit(level, item, row)`
// is called per entry with row = count, neighbours.
template <class F>
inline void for_each_entry(const FlatGraph &g, F &&emit) {
  for (int64_t i = 0; i < g.n; ++i) {
    const uint32_t *row = &g.adj0[(size_t)i * (g.m0 + 1)];
    if (g.has0[(size_t)i] || row[0] > 0) emit(0, i, row);
  }
  std::vector<int64_t> slot_item((size_t)g.slots(), -1);  // the inverse of upper_slot
  int top_all = 0;
  for (int64_t i = 0; i < g.n; ++i)
    if (g.upper_slot[(size_t)i] >= 0) slot_item[(size_t)g.upper_slot[(size_t)i]] = i;
  for (int64_t s = 0; s < g.slots(); ++s) top_all = std::max(top_all, g.upper_base[(size_t)s + 1] - g.upper_base[(size_t)s]);
  for (int l = 1; l <= top_all; ++l)
    for (int64_t s = 0; s < g.slots(); ++s) {
      const int64_t r = g.upper_base[(size_t)s] + l - 1;
      if (r >= g.upper_base[(size_t)s + 1]) continue;
      const uint32_t *row = &g.upper_adj[(size_t)r * (g.m + 1)];
      if (g.has_up[(size_t)r] || row[0] > 0) emit(l, slot_item[(size_t)s], row);
    }
}

inline void count_entries(const FlatGraph &g, int64_t *n_entries, int64_t *n_neighbours) {
  *n_entries = *n_neighbours = 0;
  for_each_entry(g, [&](int, int64_t, const uint32_t *row) {
    ++*n_entries;
    *n_neighbours += row[0];
  });
}

// into arrays of count_entries' sizes (entry_offsets: one more); entry_neighbours may be NULL when there are no neighbours
inline void emit_entries(const FlatGraph &g, int32_t *entry_level, int64_t *entry_item, int64_t *entry_offsets, int64_t *entry_neighbours) {
  int64_t e = 0, pos = 0;
  entry_offsets[0] = 0;
  for_each_entry(g, [&](int level, int64_t item, const uint32_t *row) {
    entry_level[e] = level;
    entry_item[e] = item;
    for (uint32_t k = 0; k < row[0]; ++k) entry_neighbours[pos++] = row[1 + k];
    entry_offsets[++e] = pos;
  });
}

}  // namespace hnsw_graph
