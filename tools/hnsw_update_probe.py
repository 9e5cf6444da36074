"""What updating rows in place costs (hnsw_index_update), against rebuilding.  One JSON line per configuration:
  update   per corpus, fraction of rows updated and batch: updates/s, distance evaluations per update, rounds, relinks and
           superseded relinks (hnsw_index_update_stats), recall@10 (ef = 100) of the updated index against exhaustive search
           on the new rows, beside the same of a fresh device build of the new rows and the time of that build
           (update_vs_rebuild = update seconds / rebuild seconds: above 1 the rebuild is cheaper)
The updated rows get new embeddings: i.i.d. N(0,1) rows are redrawn; rows of the Gaussian mixture move to another centre.
Corpora: i.i.d. N(0,1) and a mixture of 1000 Gaussians, d = 256, maxM = 16, efConstruction = 200, Cosine (as
tools/hnsw_append_probe.py).  --trace: one update (clustered, 1 %, batch 1024) only, the shape a kernel trace wants."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402


def corpus(kind, n, d, rng, centres):
    if kind == "iid":
        return rng.standard_normal((n, d), dtype=np.float32), None
    lab = rng.integers(0, len(centres), n)
    out = np.empty((n, d), np.float32)
    for s in range(0, n, 1 << 20):
        e = min(n, s + (1 << 20))
        out[s:e] = centres[lab[s:e]] + 0.6 * rng.standard_normal((e - s, d), dtype=np.float32)
    return out, lab


def emit(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--corpora", default="iid,clustered")
    ap.add_argument("--fractions", default="0.01,0.1")
    ap.add_argument("--batches", default="256,1024,4096")
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    if a.trace:
        a.corpora, a.fractions, a.batches = "clustered", "0.01", "1024"
    pkg = load_package()
    Hnsw, m = pkg.hnsw_ann.Hnsw, pkg.dense_ann.DistanceMetric.Cosine
    n, d, M, efc = a.n, a.dim, 16, 200
    centres = np.random.default_rng(12345).standard_normal((1000, d), dtype=np.float32)
    for kind in a.corpora.split(","):
        rng = np.random.default_rng(n + len(kind))
        x, lab = corpus(kind, n, d, rng, centres)
        qc = np.random.default_rng(7)
        q = corpus(kind, a.queries, d, qc, centres)[0]
        for frac in [float(f) for f in a.fractions.split(",")]:
            nu = int(round(frac * n))
            moved = np.sort(rng.permutation(n)[:nu]).astype(np.int64)
            rng.shuffle(moved)  # request order: random
            y = x.copy()
            if kind == "iid":
                y[moved] = rng.standard_normal((nu, d), dtype=np.float32)
            else:
                to = (lab[moved] + 1 + rng.integers(0, len(centres) - 1, nu)) % len(centres)
                y[moved] = centres[to] + 0.6 * rng.standard_normal((nu, d), dtype=np.float32)
            truth = None
            fresh_recall = rebuild_s = None
            if not a.trace:
                bf = pkg.dense_ann.BruteForceIndex.build(m, y)
                truth, _, _ = bf.search(q, 10)
                bf.close()
                t0 = time.perf_counter()
                fresh = Hnsw.build(m, y, max_m=M, ef_construction=efc, seed=1, gpu=True)
                rebuild_s = time.perf_counter() - t0

            def recall(index):
                ids, _, cnt = index.search(q, 10, 100)
                return float(np.mean([len(set(ids[i, :cnt[i]]) & set(truth[i])) / 10 for i in range(len(q))]))

            if not a.trace:
                fresh_recall = recall(fresh)
                fresh.close()
            for b in [int(s) for s in a.batches.split(",")]:
                ix = Hnsw.build(m, x, max_m=M, ef_construction=efc, seed=1, gpu=True)
                t0 = time.perf_counter()
                ix.update(y[moved], moved, ef_construction=efc, batch=b)
                t_upd = time.perf_counter() - t0
                st = ix.update_stats()
                emit(what="update", corpus=kind, n=n, d=d, fraction=frac, updates=nu, batch=b, update_s=t_upd,
                     updates_per_s=nu / t_upd, distance_evals_per_update=st["distance_evals"] / nu, rounds=st["rounds"],
                     relinks=st["relinks"], relinks_superseded=st["relinks_superseded"],
                     additions_already_present=st["additions_already_present"], lists_kept=st["lists_kept"],
                     recall10_updated=None if a.trace else recall(ix), recall10_fresh_build=fresh_recall, rebuild_s=rebuild_s,
                     update_vs_rebuild=None if a.trace else t_upd / rebuild_s)
                ix.close()
            del y
        del x


if __name__ == "__main__":
    main()
