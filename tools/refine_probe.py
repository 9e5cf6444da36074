"""What re-ranking by stored rows costs and finds (include/refine_ann.h), beside plain IVF-PQ and IVF-Flat with the same nlist,
training rows, niter and seed and against the exhaustive index, on the same rows in the same process.  One process per
(corpus, n); one JSON line per (k, nprobe, k_factor), k * k_factor <= 1024 (larger products are skipped):
  bytes_per_row          device bytes the refined index keeps per row (the base's and 2 d for the stored halves), with
                         pq_bytes_per_row and flat_bytes_per_row beside it
  refine_qps             queries/s of refine_search (best of --reps batches of nq queries), with base_ms (the base's search
                         for the k * k_factor candidates) and rerank_ms (query preparation, gather, distances, sort)
  gathered_mb            nq * k * k_factor * 2 d bytes: what the re-rank reads from the store
  recall                 recall@k against dann_search (|found & true| / |true|, averaged); pq_recall and flat_recall are those
                         of ivfpq_search and ivf_search at the same (k, nprobe), pq_qps / flat_qps their rates
Corpora and nlist as tools/ivf_probe.py; --nlist overrides.  --opq D_OUT puts the OPQ transform in front of the base.
--phases-only leaves the yardsticks out (the exhaustive index, IVF-Flat and the plain base: none of them takes rows wider
than 512) and with them recall and the *_qps beside: what is left is refine_qps, base_ms and rerank_ms, at any --dim.

Nobody has run this on a card yet: whoever does writes the numbers into DESIGN.md section 5 and profiles/.  Run each setting
under its own time limit, e.g.
  timeout -k 10 900 python tools/refine_probe.py --n 1000000 --nlist 1024 --M 32 --nprobes 32 > profiles/refine_probe_1M.jsonl"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ivf_probe import best_time, corpus  # noqa: E402
from ivfpq_probe import recall_of  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", default="clustered", choices=["clustered", "iid"])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--nlist", type=int, default=0)
    ap.add_argument("--M", type=int, default=32)
    ap.add_argument("--opq", type=int, default=0, help="d_out of an OPQ transform in front of the base (0: none)")
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--ks", default="10,64")
    ap.add_argument("--nprobes", default="32")
    ap.add_argument("--k-factors", default="1,2,4,8,16")
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--niter-opq", type=int, default=10)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--metric", default="L2")
    ap.add_argument("--phases-only", action="store_true", help="no yardsticks and no recall: the phase times alone")
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
    k_factors = [int(s) for s in a.k_factors.split(",")]

    truth, dense_s = {}, {}
    if not a.phases_only:
        dense = pkg.dense_ann.BruteForceIndex.build(m, x)
        for k in ks:
            dense.search(q, k)
            dense_s[k], truth[k] = best_time(lambda: dense.search(q, k), a.reps)
        dense.close()

    def train_base():
        if a.opq:
            return pkg.opq_ann.FaissOpqIvfPq.train(m, nlist, a.M, a.opq, x[:n_train], niter=a.niter, niter_opq=a.niter_opq, seed=1)
        return pkg.ivfpq_ann.FaissIvfPq.train(m, nlist, a.M, x[:n_train], niter=a.niter, seed=1)

    # the two yardsticks of the same run: IVF-Flat and the plain base
    beside = {}
    for name, make in () if a.phases_only else (("flat", lambda: pkg.ivf_ann.FaissIvfFlat.train(m, nlist, x[:n_train], niter=a.niter, seed=1)), ("pq", train_base)):
        ix = make()
        t0 = time.perf_counter()
        ix.add(x)
        add_s = time.perf_counter() - t0
        for k in ks:
            for nprobe in nprobes:
                ix.search(q, k, nprobe)
                s, (ids, _, cnt) = best_time(lambda: ix.search(q, k, nprobe), a.reps)
                beside.setdefault((k, nprobe), {}).update({
                    f"{name}_add_s": round(add_s, 3), f"{name}_qps": round(len(q) / s, 1), f"{name}_ms": round(s * 1e3, 3),
                    f"{name}_bytes_per_row": ix.bytes_per_row() if name == "pq" else 4 * d + 24,
                    f"{name}_recall": round(recall_of(ids, cnt, truth[k][0], truth[k][2]), 4)})
        ix.close()

    t0 = time.perf_counter()
    ix = pkg.refine_ann.FaissRefineFlat.wrap(train_base())
    train_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    ix.add(x)
    add_s = time.perf_counter() - t0
    for k in ks:
        for nprobe in nprobes:
            for kf in k_factors:
                if k * kf > pkg.refine_ann.MAX_CANDIDATES:
                    continue
                ix.search(q, k, nprobe, kf)  # warm-up
                s, (ids, _, cnt) = best_time(lambda: ix.search(q, k, nprobe, kf), a.reps)
                st = ix.last_stats()
                line = {
                    "corpus": a.corpus, "metric": a.metric, "n": n, "d": d, "nlist": nlist, "M": a.M, "opq_d_out": a.opq,
                    "n_train": n_train, "niter": a.niter, "sigma": a.sigma, "nq": len(q), "k": k, "nprobe": nprobe, "k_factor": kf,
                    "train_s": round(train_s, 3), "add_s": round(add_s, 3), "bytes_per_row": ix.bytes_per_row(),
                    "refine_qps": round(len(q) / s, 1), "refine_ms": round(s * 1e3, 3), "base_ms": round(st["base_ms"], 3),
                    "rerank_ms": round(st["rerank_ms"], 3), "gathered_mb": round(len(q) * k * kf * 2 * d / 1e6, 3)}
                if not a.phases_only:
                    line.update({"dense_qps": round(len(q) / dense_s[k], 1),
                                 "recall": round(recall_of(ids, cnt, truth[k][0], truth[k][2]), 4)})
                    line.update(beside[(k, nprobe)])
                print(json.dumps(line), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
