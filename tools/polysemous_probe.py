"""What the Hamming filter of polysemous codes costs and finds (include/polysemous_ann.h): a plain and a polysemous IVF-PQ
index with the same nlist, M, training rows, niter and seed on one synthetic set, in the same process.  One JSON line per
(index, k, nprobe, ht):
  scan_ms                HIP-event milliseconds of the scan rounds of the last of --reps searches (ivfpq_last_stats), with
                         search_ms, the best wall-clock time of a whole search of nq queries
  scored_ratio           rows_scored / rows_scanned: the share of the rows read that passed the filter and did their M lookups
  recall_vs_unfiltered   recall@k against the same index searched without a filter (ht = 0)
  recall                 recall@k against dann_search, the exhaustive index
ht = 0 is the unfiltered search.  On the plain index the filter runs over codes whose numbering means nothing: the line beside
the polysemous one is what the renumbering buys.  Corpora and nlist as tools/ivf_probe.py; --nlist overrides.

Nobody has run this on a card yet: whoever does writes the numbers into DESIGN.md section 5 and profiles/.  Run each setting
under its own time limit, e.g.
  timeout -k 10 900 python tools/polysemous_probe.py --n 1000000 --nlist 1024 --M 48 --dim 240 > profiles/polysemous_probe_1M.jsonl"""
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
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--ks", default="10")
    ap.add_argument("--nprobes", default="32")
    ap.add_argument("--hts", default="", help="comma-separated thresholds; default: 0 and 4M - 4 sqrt(2M) .. 4M + 2 sqrt(2M)")
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--anneal-iters", type=int, default=0)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--metric", default="L2")
    a = ap.parse_args()
    pkg = load_package()
    ps = pkg.polysemous_ann
    m = getattr(pkg.dense_ann.DistanceMetric, a.metric)
    n, d, M = a.n, a.dim, a.M
    nlist = a.nlist or 1 << round(math.log2(4 * math.sqrt(n)))
    x, q = corpus(a.corpus, n, d, nlist // 4, a.sigma, n + len(a.corpus))
    q = q[:a.nq]
    n_train = min(n, 64 * nlist)
    ks = [int(s) for s in a.ks.split(",")]
    nprobes = [int(s) for s in a.nprobes.split(",")]
    if a.hts:
        hts = [int(s) for s in a.hts.split(",")]
    else:  # around the mean 4M of the Hamming distance of two random codes, in steps of its deviation sqrt(2M)
        dev = math.sqrt(2 * M)
        hts = [0] + sorted({max(1, round(4 * M + s * dev)) for s in (-4, -3, -2, -1, 0, 1, 2)})

    dense = pkg.dense_ann.BruteForceIndex.build(m, x)
    truth = {}
    for k in ks:
        truth[k] = dense.search(q, k)
    dense.close()

    for name in ("plain", "polysemous"):
        t0 = time.perf_counter()
        if name == "plain":
            ix = ps.adopt(pkg.ivfpq_ann.FaissIvfPq.train(m, nlist, M, x[:n_train], niter=a.niter, seed=1))
        else:
            ix = ps.PolysemousIvfPq.train(m, nlist, M, x[:n_train], niter=a.niter, seed=1, anneal_iters=a.anneal_iters)
        train_s = time.perf_counter() - t0
        ix.add(x)
        for k in ks:
            for nprobe in nprobes:
                base_ids, _, base_cnt = ix.search(q, k, nprobe, 0)
                for ht in hts:
                    ix.search(q, k, nprobe, ht)  # warm-up
                    s, (ids, _, cnt) = best_time(lambda: ix.search(q, k, nprobe, ht), a.reps)
                    st, scored = ix.last_stats(), ix.last_ht_stats()["rows_scored"]
                    print(json.dumps({
                        "index": name, "corpus": a.corpus, "metric": a.metric, "n": n, "d": d, "nlist": nlist, "M": M, "n_train": n_train,
                        "niter": a.niter, "anneal_iters": a.anneal_iters or ps.DEFAULT_ANNEAL_ITERS, "sigma": a.sigma, "nq": len(q),
                        "k": k, "nprobe": nprobe, "ht": ht, "train_s": round(train_s, 3), "search_ms": round(s * 1e3, 3),
                        "scan_ms": round(st["scan_ms"], 3), "rounds": st["rounds"], "rows_scanned": st["rows_scanned"],
                        "rows_scored": scored, "scored_ratio": round(scored / max(st["rows_scanned"], 1), 5),
                        "mean_count": round(float(np.mean(cnt)), 3),
                        "recall_vs_unfiltered": round(recall_of(ids, cnt, base_ids, base_cnt), 4),
                        "recall": round(recall_of(ids, cnt, truth[k][0], truth[k][2]), 4)}), flush=True)
        ix.close()


if __name__ == "__main__":
    main()
