"""What the IVF-Flat index costs and finds (include/ivf_ann.h), against the exhaustive index on the same rows in the same
process.  One process per (corpus, n); one JSON line per (k, nprobe):
  train_s / add_s   ivf_index_train on the first min(n, 64 nlist) rows (niter rounds), ivf_index_add of all rows
  ivf_qps           queries/s of ivf_search (best of --reps batches of nq queries), and its coarse / scan / select milliseconds
  dense_qps         queries/s of dann_search on the same rows and batch
  rows_scanned      the sum over the batch of the sizes of the probed lists; bytes_raw = rows_scanned * d * 2 is what a
                    scan that read a list once per query would move, bytes_shared = the blocks the scan's workgroups read
                    (a list is read once per group of <= 32 queries that probe it); hbm_frac_* = bytes / scan time / peak
  recall            recall@k against dann_search (the load test's definition: |found & true| / |true|, averaged)
Corpora: `clustered` = a mixture of nlist/4 Gaussians (sigma --sigma), `iid` = N(0,1) (BASELINE configs[3]), where every
cell is about as far as every other and a large nprobe is needed.  nlist = 4 sqrt(n) rounded to a power of two.

Run each setting under its own time limit and chain them, e.g.
  timeout -k 10 900 python tools/ivf_probe.py --corpus clustered --n 1000000 > profiles/r07_ivf_probe_clustered_1M.jsonl && \\
  timeout -k 10 900 python tools/ivf_probe.py --corpus iid --n 1000000 > profiles/r07_ivf_probe_iid_1M.jsonl"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X


def corpus(kind, n, d, n_clusters, sigma, seed):
    rng = np.random.default_rng(seed)
    if kind == "iid":
        return rng.standard_normal((n, d), dtype=np.float32), rng.standard_normal((4096, d), dtype=np.float32)
    centres = np.random.default_rng(12345).standard_normal((n_clusters, d), dtype=np.float32)
    out = np.empty((n, d), np.float32)
    for s in range(0, n, 1 << 20):
        e = min(n, s + (1 << 20))
        out[s:e] = centres[rng.integers(0, n_clusters, e - s)] + sigma * rng.standard_normal((e - s, d), dtype=np.float32)
    q = centres[rng.integers(0, n_clusters, 4096)] + sigma * rng.standard_normal((4096, d), dtype=np.float32)
    return out, q


def best_time(fn, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", default="clustered", choices=["clustered", "iid"])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--ks", default="10,200")
    ap.add_argument("--nprobes", default="1,8,32,128")
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--metric", default="L2")
    a = ap.parse_args()
    pkg = load_package()
    m = getattr(pkg.dense_ann.DistanceMetric, a.metric)
    n, d = a.n, a.dim
    nlist = 1 << round(math.log2(4 * math.sqrt(n)))
    x, q = corpus(a.corpus, n, d, nlist // 4, a.sigma, n + len(a.corpus))
    q = q[:a.nq]
    n_train = min(n, 64 * nlist)
    t0 = time.perf_counter()
    ix = pkg.ivf_ann.FaissIvfFlat.train(m, nlist, x[:n_train], niter=a.niter, seed=1)
    train_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    ix.add(x)
    add_s = time.perf_counter() - t0
    sizes = ix.list_sizes()
    dense = pkg.dense_ann.BruteForceIndex.build(m, x)
    del x
    for k in [int(s) for s in a.ks.split(",")]:
        dense.search(q, k)  # warm-up
        dense_s, (t_ids, _, t_cnt) = best_time(lambda: dense.search(q, k), a.reps)
        for nprobe in [int(s) for s in a.nprobes.split(",")]:
            ix.search(q, k, nprobe)  # warm-up
            ivf_s, (ids, _, cnt) = best_time(lambda: ix.search(q, k, nprobe), a.reps)
            st = ix.last_stats()
            probes = ix.last_probes()
            # blocks the scan's workgroups read: per cell, ceil(queries probing it / 32) passes over its ceil(size / 32) blocks
            per_cell = np.bincount(probes.ravel(), minlength=nlist)
            shared_rows = int((((per_cell + 31) // 32) * ((sizes + 31) // 32) * 32).sum()) * st["rounds"]
            recall = float(np.mean([len(set(ids[i, :cnt[i]].tolist()) & set(t_ids[i, :t_cnt[i]].tolist())) / max(1, t_cnt[i])
                                    for i in range(len(q))]))
            scan_s = max(st["scan_ms"], 1e-6) * 1e-3
            print(json.dumps({
                "corpus": a.corpus, "metric": a.metric, "n": n, "d": d, "nlist": nlist, "n_train": n_train, "niter": a.niter,
                "sigma": a.sigma, "nq": len(q), "k": k, "nprobe": nprobe, "train_s": round(train_s, 3), "add_s": round(add_s, 3),
                "list_size_min": int(sizes.min()), "list_size_max": int(sizes.max()),
                "ivf_qps": round(len(q) / ivf_s, 1), "dense_qps": round(len(q) / dense_s, 1),
                "ivf_ms": round(ivf_s * 1e3, 3), "dense_ms": round(dense_s * 1e3, 3),
                "coarse_ms": round(st["coarse_ms"], 3), "scan_ms": round(st["scan_ms"], 3), "select_ms": round(st["select_ms"], 3),
                "rounds": st["rounds"], "rows_scanned": st["rows_scanned"],
                "bytes_raw": st["rows_scanned"] * d * 2, "bytes_shared": shared_rows * d * 2,
                "hbm_frac_raw": round(st["rows_scanned"] * d * 2 / scan_s / HBM_PEAK, 4),
                "hbm_frac_shared": round(shared_rows * d * 2 / scan_s / HBM_PEAK, 4),
                "recall": round(recall, 4)}), flush=True)
    ix.close()
    dense.close()


if __name__ == "__main__":
    main()
