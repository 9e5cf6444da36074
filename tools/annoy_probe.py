"""The comparison of the reference's experimental/Runner.scala (:18-57) on the device: an Annoy index of 80 trees over
Cosine, nodesToExplore over the Runner's list (0 .. 50,000), against HNSW (efConstruction 200, maxM 16, ef over the
Runner's list) and the exhaustive search, on the same rows in the same process.  The Runner's data by default: 300
dimensions, rows uniform in [0, 50), queries uniform in [0, 1), 20 neighbours; --n and --nq scale it (the Runner has 2000
rows and 30 queries), --corpus lowdim takes rows with 3 latent dimensions instead.  One JSON line per setting:
  kind annoy   nodes_to_explore, search_k, ms (best of --reps batches of nq queries), qps, walk_ms / score_ms / select_ms
               (HIP events of the last batch), pops and candidates per query (mean), rerun, slices, recall
  kind hnsw    ef, ms, qps, recall
  kind brute   ms, qps
recall is |found & true| / k against the exhaustive search, averaged, as the Runner counts it.  build_s is the host build of
the forest with --threads threads.  --phases-only leaves the exhaustive search out (it takes no rows wider than 512) and
with it recall and HNSW: the Annoy lines alone, at any --dim.  Run under a time limit, e.g.
  timeout -k 10 600 python tools/annoy_probe.py --n 100000 --nq 1024 > profiles/annoy_probe_100k.jsonl"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ivf_probe import best_time  # noqa: E402
from ivfpq_probe import recall_of  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

NODES_TO_EXPLORE = [0, 2000, 3000, 5000, 7000, 10000, 15000, 20000, 30000, 35000, 40000, 50000]  # Runner.scala:38-39
EF_SEARCH = [20, 30, 50, 70, 100, 120]                                                          # Runner.scala:31-32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--nq", type=int, default=30)
    ap.add_argument("--dim", type=int, default=300)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--trees", type=int, default=80)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--corpus", default="runner", choices=["runner", "lowdim"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-hnsw", action="store_true")
    ap.add_argument("--phases-only", action="store_true", help="no exhaustive search, no recall, no HNSW: the Annoy lines alone")
    a = ap.parse_args()
    pkg = load_package()
    cosine = pkg.dense_ann.DistanceMetric.Cosine
    rng = np.random.default_rng(1)
    if a.corpus == "runner":
        x = (rng.random((a.n, a.dim)) * 50).astype(np.float32)
        q = rng.random((a.nq, a.dim)).astype(np.float32)
    else:
        basis = rng.standard_normal((3, a.dim)) / np.sqrt(3)
        y = (rng.standard_normal((a.n + a.nq, 3)) @ basis + 0.3 * rng.standard_normal((a.n + a.nq, a.dim))).astype(np.float32)
        x, q = y[:a.n], y[a.n:]
    common = {"corpus": a.corpus, "n": a.n, "d": a.dim, "nq": a.nq, "k": a.k}

    truth = None
    if not a.phases_only:
        dense = pkg.dense_ann.BruteForceIndex.build(cosine, x, np.arange(1, a.n + 1))
        dense.search(q, a.k)
        s, truth = best_time(lambda: dense.search(q, a.k), a.reps)
        dense.close()
        print(json.dumps(dict(common, kind="brute", ms=round(s * 1e3, 3), qps=round(a.nq / s, 1))), flush=True)

    t0 = time.perf_counter()
    forest = pkg.annoy_ann.AnnoyForest.build(cosine, x, a.trees, threads=a.threads)
    build_s = time.perf_counter() - t0
    ix = pkg.annoy_ann.AnnoyQueryable.from_forest(forest, x)
    info = ix.info()
    for nte in NODES_TO_EXPLORE:
        search_k = a.trees * max(a.k, nte // a.trees)
        ix.search(q, a.k, nte)  # warm-up
        s, (ids, _, cnt) = best_time(lambda: ix.search(q, a.k, nte), a.reps)
        st = ix.last_stats()
        _, ccnt = ix.last_candidates()
        print(json.dumps(dict(common, kind="annoy", trees=a.trees, leaf_size=info["leaf_size"], n_nodes=info["n_nodes"],
                              build_s=round(build_s, 3), nodes_to_explore=nte, search_k=search_k, ms=round(s * 1e3, 3),
                              qps=round(a.nq / s, 1), walk_ms=round(st["walk_ms"], 3), score_ms=round(st["score_ms"], 3),
                              select_ms=round(st["select_ms"], 3), pops=round(float(st["pops"].mean()), 1),
                              candidates=round(float(ccnt.mean()), 1), rerun=st["rerun"], slices=st["slices"],
                              recall=round(recall_of(ids, cnt, truth[0], truth[2]), 4) if truth else None)), flush=True)
    ix.close()
    forest.close()

    if not a.no_hnsw and not a.phases_only:
        t0 = time.perf_counter()
        hn = pkg.hnsw_ann.Hnsw.build(cosine, x, np.arange(1, a.n + 1), max_m=16, ef_construction=200, n_threads=16)
        hbuild_s = time.perf_counter() - t0
        for ef in EF_SEARCH:
            hn.search(q, a.k, max(ef, a.k))
            s, (ids, _, cnt) = best_time(lambda: hn.search(q, a.k, max(ef, a.k)), a.reps)
            print(json.dumps(dict(common, kind="hnsw", ef=ef, build_s=round(hbuild_s, 3), ms=round(s * 1e3, 3), qps=round(a.nq / s, 1),
                                  recall=round(recall_of(ids, cnt, truth[0], truth[2]), 4))), flush=True)
        hn.close()


if __name__ == "__main__":
    main()
