// hnsw_host_builder.h -- the reference's insertion algorithm on host threads (hnsw_index_build_insert; HnswIndex.java:137-200,
// 384-440, 479-526): the graph under construction, the stored rows as the host reads them, DistancedItemQueue, the insert
// itself, and the result as the FlatGraph the index keeps.  Included once, by hnsw_ann.hip; everything is file-local.
#pragma once
#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "hnsw_graph_host.h"
#include "hnsw_queue.h"

namespace {

// graph under construction.  Dense rows: item i owns rows base[i] .. base[i] + top[i] (levels
// 0..top[i]); `has` says whether the reference's map holds the key HnswNode(level, item) at all.
// One lock per stripe of items guards a row's read-modify-write, so the builder can run on several
// host threads (the reference inserts concurrently too, HnswIndex.java:150-200); at most one lock is
// ever held, so there is nothing to deadlock on.
struct HostGraph {
  int64_t n = 0;
  int m = 0, m0 = 0;
  int max_level = -1;  // HnswIndex.java:97
  int64_t entry = -1;
  std::vector<int32_t> top;
  std::vector<int64_t> base;
  std::vector<std::vector<uint32_t>> rows;
  std::vector<uint8_t> has;
  std::unique_ptr<std::mutex[]> locks;
  static constexpr size_t STRIPES = 8192;
  std::mutex meta;

  void init(int64_t n_, int m_, const std::vector<int32_t> &tops) {
    n = n_;
    m = m_;
    m0 = 2 * m_;
    top = tops;
    base.assign((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) base[(size_t)i + 1] = base[(size_t)i] + top[(size_t)i] + 1;
    rows.assign((size_t)base[(size_t)n], {});
    has.assign((size_t)base[(size_t)n], 0);
    locks.reset(new std::mutex[STRIPES]);
  }
  std::mutex &lock_of(uint32_t item) { return locks[item % STRIPES]; }
  // getConnectionListForRead: a copy of the list, empty when the key is absent
  std::vector<uint32_t> read(int level, uint32_t item) {
    if (level > top[item]) return {};
    std::lock_guard<std::mutex> lk(lock_of(item));
    return rows[(size_t)(base[item] + level)];
  }
  bool exists(int level, uint32_t item) const { return level <= top[item] && has[(size_t)(base[item] + level)]; }
  void put_locked(int level, uint32_t item, std::vector<uint32_t> list) {  // caller holds lock_of(item)
    rows[(size_t)(base[item] + level)] = std::move(list);
    has[(size_t)(base[item] + level)] = 1;
  }
  void put(int level, uint32_t item, std::vector<uint32_t> list) {
    std::lock_guard<std::mutex> lk(lock_of(item));
    put_locked(level, item, std::move(list));
  }
};

// stored rows on the host, fp16-rounded, each 64-element block transposed ([e][j] instead of [j][e]) so that
// the 8 partial sums of the fixed summation order are the lanes of one SIMD accumulator
struct HostVectors {
  std::vector<float> t;
  int dpad = 0, metric = 0;
  void load(const std::vector<float> &rows, int64_t n, int dpad_, int metric_) {
    dpad = dpad_;
    metric = metric_;
    t.resize(rows.size());
    for (int64_t i = 0; i < n; ++i)
      for (int b = 0; b < dpad / 64; ++b)
        for (int j = 0; j < 8; ++j)
          for (int e = 0; e < 8; ++e) t[(size_t)i * dpad + b * 64 + e * 8 + j] = rows[(size_t)i * dpad + b * 64 + j * 8 + e];
  }
  float distance(uint32_t a, uint32_t b) const {
    const float *q = t.data() + (size_t)a * dpad, *y = t.data() + (size_t)b * dpad;
    float p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (metric == HNSW_METRIC_L2) {
      for (int k = 0; k < dpad; k += 8)
        for (int j = 0; j < 8; ++j) {
          const float d = q[k + j] - y[k + j];
          p[j] = p[j] + d * d;
        }
    } else {
      for (int k = 0; k < dpad; k += 8)
        for (int j = 0; j < 8; ++j) p[j] = p[j] + q[k + j] * y[k + j];
    }
    const float r0 = p[0] + p[1], r2 = p[2] + p[3], r4 = p[4] + p[5], r6 = p[6] + p[7];
    return finish_distance(metric, (r0 + r2) + (r4 + r6));
  }
};

// DistancedItemQueue on the host
struct JQueue {
  std::vector<HEntry> q;
  int n = 0;
  bool minq;
  uint32_t origin;
  explicit JQueue(bool mq, uint32_t o) : minq(mq), origin(o) {}
  void add(HEntry e) {
    if ((int)q.size() <= n) q.resize((size_t)n + 64);
    if (minq) pq_add<true>(q.data(), n, e);
    else pq_add<false>(q.data(), n, e);
  }
  HEntry poll() { return minq ? pq_poll<true>(q.data(), n) : pq_poll<false>(q.data(), n); }
  JQueue reverse() const {  // DistancedItemQueue.reverse: re-add in array (iterator) order
    JQueue r(!minq, origin);
    for (int i = 0; i < n; ++i) r.add(q[(size_t)i]);
    return r;
  }
};

struct Builder {  // one per host thread
  HostGraph &g;
  const HostVectors &v;
  int ef_construction;
  std::vector<uint32_t> stamp;  // visited set, epoch-stamped
  uint32_t epoch = 0;

  uint32_t best_entry(uint32_t entry, uint32_t item, int max_layer, int selected) {  // HnswIndex.java:447-475
    uint32_t cur = entry;
    if (selected < max_layer) {
      float cur_dist = v.distance(item, cur);
      for (int level = max_layer; level > selected; --level) {
        bool changed = true;
        while (changed) {
          changed = false;
          for (uint32_t nn : g.read(level, cur)) {
            const float t = v.distance(item, nn);
            if (t < cur_dist) {
              cur_dist = t;
              cur = nn;
              changed = true;
            }
          }
        }
      }
    }
    return cur;
  }

  JQueue search_layer(uint32_t item, uint32_t entry, int ef, int level) {  // HnswIndex.java:571-623, isUpdate = false
    JQueue cq(true, item);
    cq.add(HEntry{v.distance(item, entry), entry});
    JQueue wq = cq.reverse();
    ++epoch;
    stamp[entry] = epoch;
    float lower = wq.q[0].dist;
    while (cq.n > 0) {
      const HEntry cand = cq.q[0];
      if (cand.dist > lower) break;
      cq.poll();
      for (uint32_t nn : g.read(level, cand.node)) {
        if (stamp[nn] == epoch) continue;
        stamp[nn] = epoch;
        const float dist = v.distance(item, nn);
        if (wq.n < ef || dist < wq.q[0].dist) {
          cq.add(HEntry{dist, nn});
          wq.add(HEntry{dist, nn});
          if (wq.n > ef) wq.poll();
          lower = wq.q[0].dist;
        }
      }
    }
    return wq;
  }

  std::vector<uint32_t> select(const JQueue &cands, int max_conn) {  // HnswIndex.java:479-526
    const uint32_t base = cands.origin;
    std::vector<uint32_t> res;
    if (cands.n <= max_conn) {
      bool removed = false;  // List.remove(Object): first occurrence only
      for (int i = 0; i < cands.n; ++i) {
        if (!removed && cands.q[(size_t)i].node == base) {
          removed = true;
          continue;
        }
        res.push_back(cands.q[(size_t)i].node);
      }
      return res;
    }
    JQueue minq = cands.reverse();
    while (minq.n > 0) {
      if ((int)res.size() >= max_conn) break;
      const HEntry c = minq.poll();
      if (c.node == base) continue;
      bool include = true;
      for (uint32_t e : res) {
        if (v.distance(e, c.node) < c.dist) {
          include = false;
          break;
        }
      }
      if (include) res.push_back(c.node);
    }
    return res;
  }

  uint32_t connect(uint32_t item, const JQueue &cands, int level) {  // mutuallyConnectNewElement, isUpdate = false
    const std::vector<uint32_t> neighbours = select(cands, g.m);
    g.put(level, item, neighbours);
    const int M = level == 0 ? g.m0 : g.m;
    for (uint32_t nn : neighbours) {
      if (nn == item) continue;
      std::lock_guard<std::mutex> lk(g.lock_of(nn));  // the neighbour's write lock (:406-435)
      std::vector<uint32_t> conn = g.rows[(size_t)(g.base[nn] + level)];
      if ((int)conn.size() < M) {
        conn.push_back(item);
      } else {
        JQueue q(false, nn);
        for (uint32_t t : conn) q.add(HEntry{v.distance(nn, t), t});
        q.add(HEntry{v.distance(nn, item), item});
        conn = select(q, M);
      }
      g.put_locked(level, nn, std::move(conn));
    }
    return neighbours.empty() ? item : neighbours[0];
  }

  void insert(uint32_t item, int cur_level) {  // HnswIndex.java:137-200
    int64_t entry;
    int max_layer;
    bool hold_meta = false;
    g.meta.lock();
    entry = g.entry;
    max_layer = g.max_level;
    if (cur_level > max_layer) hold_meta = true;  // the global lock: this insert may move the entry point (:173-183)
    else g.meta.unlock();
    if (entry >= 0) {
      uint32_t cur = (uint32_t)entry;
      if (cur_level < max_layer) cur = best_entry(cur, item, max_layer, cur_level);
      for (int level = std::min(cur_level, max_layer); level >= 0; --level) {
        const JQueue cands = search_layer(item, cur, ef_construction, level);
        cur = connect(item, cands, level);
      }
    }
    if (hold_meta) {  // HnswMeta starts at (-1, empty): the first item always takes this branch
      g.max_level = cur_level;
      g.entry = item;
      g.meta.unlock();
    }
  }
};

// items 0..n-1 at the given levels into g (initialised with them), on n_threads host threads
void insert_all(HostGraph &g, const HostVectors &hv, int ef_construction, const std::vector<int32_t> &levels, int32_t n_threads) {
  const int64_t n = g.n;
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(n_threads, std::max<int64_t>(1, n / 64)));
  if (nt == 1) {
    Builder b{g, hv, ef_construction, std::vector<uint32_t>((size_t)n, 0), 0};
    for (int64_t i = 0; i < n; ++i) b.insert((uint32_t)i, levels[(size_t)i]);
  } else {
    // the first items go in one by one (an entry point must exist), the rest concurrently
    const int64_t warm = std::min<int64_t>(n, 256);
    {
      Builder b{g, hv, ef_construction, std::vector<uint32_t>((size_t)n, 0), 0};
      for (int64_t i = 0; i < warm; ++i) b.insert((uint32_t)i, levels[(size_t)i]);
    }
    std::atomic<int64_t> next(warm);
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; ++t)
      pool.emplace_back([&]() {
        Builder b{g, hv, ef_construction, std::vector<uint32_t>((size_t)n, 0), 0};
        for (;;) {
          const int64_t i = next.fetch_add(1);
          if (i >= n) break;
          b.insert((uint32_t)i, levels[(size_t)i]);
        }
      });
    for (auto &th : pool) th.join();
  }
}

// the builder's result in the form the index keeps
hnsw_graph::FlatGraph flat_graph(const HostGraph &g) {
  hnsw_graph::FlatGraph f;
  f.init(g.n, g.m, g.top);
  f.entry = g.entry;
  f.max_level = std::max(g.max_level, 0);
  for (int64_t i = 0; i < g.n; ++i)
    for (int l = 0; l <= g.top[(size_t)i]; ++l) {
      const std::vector<uint32_t> &list = g.rows[(size_t)(g.base[(size_t)i] + l)];
      uint32_t *row = f.row(l, i);
      row[0] = (uint32_t)list.size();
      std::copy(list.begin(), list.end(), row + 1);
      f.has(l, i) = g.has[(size_t)(g.base[(size_t)i] + l)];
    }
  return f;
}

}  // namespace
