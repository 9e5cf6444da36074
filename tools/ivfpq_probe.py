"""What the IVF-PQ index costs and finds (include/ivfpq_ann.h), against the exhaustive index and against IVF-Flat with the same
nlist, training rows, niter and seed, on the same rows in the same process.  One process per (corpus, n); one JSON line
per (M, k, nprobe):
  train_s / add_s       ivfpq_index_train on the first min(n, 64 nlist) rows (niter rounds for cells and codebooks),
                        ivfpq_index_add of all rows
  bytes_per_row         device bytes the index keeps per row (codes twice, id twice, cell, rank); flat_bytes_per_row beside it
  pq_qps                queries/s of ivfpq_search (best of --reps batches of nq queries), with its coarse / scan / select ms
  flat_*                the IVF-Flat line of the same run: train_s, add_s, qps and recall at the same (k, nprobe)
  dense_qps             queries/s of dann_search on the same rows and batch
  recall, recall_vs_flat  recall@k against dann_search and against IVF-Flat's answer (|found & true| / |true|, averaged)
Corpora and nlist as tools/ivf_probe.py; --nlist overrides.

Run each setting under its own time limit, e.g.
  timeout -k 10 900 python tools/ivfpq_probe.py --n 1000000 --nlist 1024 --Ms 16,32,64 --nprobes 32 > profiles/ivfpq_probe_1M.jsonl"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ivf_probe import best_time, corpus  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def recall_of(ids, cnt, t_ids, t_cnt):
    return float(np.mean([len(set(ids[i, :cnt[i]].tolist()) & set(t_ids[i, :t_cnt[i]].tolist())) / max(1, t_cnt[i])
                          for i in range(len(ids))]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", default="clustered", choices=["clustered", "iid"])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--nlist", type=int, default=0)
    ap.add_argument("--Ms", default="16,32,64")
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--ks", default="10,200")
    ap.add_argument("--nprobes", default="32")
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--metric", default="L2")
    a = ap.parse_args()
    pkg = load_package()
    m = getattr(pkg.dense_ann.DistanceMetric, a.metric)
    n, d = a.n, a.dim
    nlist = a.nlist or 1 << round(math.log2(4 * math.sqrt(n)))
    x, q = corpus(a.corpus, n, d, nlist // 4, a.sigma, n + len(a.corpus))
    q = q[:a.nq]
    n_train = min(n, 64 * nlist)
    ks = [int(s) for s in a.ks.split(",")]
    nprobes = [int(s) for s in a.nprobes.split(",")]

    # the two yardsticks first: the exhaustive index and IVF-Flat
    dense = pkg.dense_ann.BruteForceIndex.build(m, x)
    truth, dense_s = {}, {}
    for k in ks:
        dense.search(q, k)
        dense_s[k], truth[k] = best_time(lambda: dense.search(q, k), a.reps)
    dense.close()
    t0 = time.perf_counter()
    flat = pkg.ivf_ann.FaissIvfFlat.train(m, nlist, x[:n_train], niter=a.niter, seed=1)
    flat_train_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    flat.add(x)
    flat_add_s = time.perf_counter() - t0
    flat_line = {}
    for k in ks:
        for nprobe in nprobes:
            flat.search(q, k, nprobe)
            s, (ids, _, cnt) = best_time(lambda: flat.search(q, k, nprobe), a.reps)
            st = flat.last_stats()
            flat_line[(k, nprobe)] = (ids, cnt, {
                "flat_train_s": round(flat_train_s, 3), "flat_add_s": round(flat_add_s, 3), "flat_bytes_per_row": 4 * d + 24,
                "flat_qps": round(len(q) / s, 1), "flat_ms": round(s * 1e3, 3), "flat_scan_ms": round(st["scan_ms"], 3),
                "flat_recall": round(recall_of(ids, cnt, truth[k][0], truth[k][2]), 4)})
    flat.close()

    for M in [int(s) for s in a.Ms.split(",")]:
        t0 = time.perf_counter()
        ix = pkg.ivfpq_ann.FaissIvfPq.train(m, nlist, M, x[:n_train], niter=a.niter, seed=1)
        train_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        ix.add(x)
        add_s = time.perf_counter() - t0
        sizes = ix.list_sizes()
        for k in ks:
            for nprobe in nprobes:
                ix.search(q, k, nprobe)  # warm-up
                s, (ids, _, cnt) = best_time(lambda: ix.search(q, k, nprobe), a.reps)
                st = ix.last_stats()
                f_ids, f_cnt, f_line = flat_line[(k, nprobe)]
                line = {
                    "corpus": a.corpus, "metric": a.metric, "n": n, "d": d, "nlist": nlist, "M": M, "n_train": n_train,
                    "niter": a.niter, "sigma": a.sigma, "nq": len(q), "k": k, "nprobe": nprobe,
                    "train_s": round(train_s, 3), "add_s": round(add_s, 3), "bytes_per_row": ix.bytes_per_row(),
                    "list_size_min": int(sizes.min()), "list_size_max": int(sizes.max()),
                    "pq_qps": round(len(q) / s, 1), "pq_ms": round(s * 1e3, 3), "dense_qps": round(len(q) / dense_s[k], 1),
                    "coarse_ms": round(st["coarse_ms"], 3), "scan_ms": round(st["scan_ms"], 3), "select_ms": round(st["select_ms"], 3),
                    "rounds": st["rounds"], "rows_scanned": st["rows_scanned"],
                    "recall": round(recall_of(ids, cnt, truth[k][0], truth[k][2]), 4),
                    "recall_vs_flat": round(recall_of(ids, cnt, f_ids, f_cnt), 4)}
                line.update(f_line)
                print(json.dumps(line), flush=True)
        ix.close()


if __name__ == "__main__":
    main()
