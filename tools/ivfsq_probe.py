"""What the scalar-quantised lists cost and find (include/ivfsq_ann.h) beside the flat lists (include/ivf_ann.h): an
`IVF<nlist>,Flat` and an `IVF<nlist>,SQ8` built from the same training arguments over the same rows, in one process.  The
two must have byte-equal centroids and, for every search, equal probes: then they scan the same lists, and what differs is
the payload.  One JSON line:
  train_s / add_s            of both builds
  list_bytes_per_row         from the layout: the slots of all 32-row blocks times (payload + bias + rank) over n
  by_k[k]                    for k in --ks, over --reps alternating searches of the two indexes after a warm-up of both:
      flat / sq8             median, min and max of coarse_ms, scan_ms, select_ms (HIP events) and of the wall-clock call
      rows_scanned, rounds
      recall_sq8_vs_flat     |SQ8 top-k & Flat top-k| / |Flat top-k|, averaged over the queries
      recall_*_vs_exhaustive the same against dann_search over all rows
Corpora as in tools/ivf_probe.py.  Without a device the first library call fails: there is no fallback.

  timeout -k 10 900 python tools/ivfsq_probe.py > profiles/ivfsq_probe_1m.jsonl"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402
from tools.ivf_probe import corpus  # noqa: E402


def spread(values):
    v = np.asarray(values, np.float64)
    return {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3)}


def recall(ids, cnt, t_ids, t_cnt):
    return round(float(np.mean([len(set(ids[i, :cnt[i]].tolist()) & set(t_ids[i, :t_cnt[i]].tolist())) / max(1, t_cnt[i])
                                for i in range(len(cnt))])), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", default="clustered", choices=["clustered", "iid"])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--ks", default="10,200")
    ap.add_argument("--niter", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--metric", default="L2")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5: the spread is part of the result")
    pkg = load_package()
    import importlib
    sq = importlib.import_module(pkg.__name__ + ".scalar_quantizer")
    m = getattr(pkg.dense_ann.DistanceMetric, a.metric)
    n, d, nlist = a.n, a.dim, a.nlist
    x, q = corpus(a.corpus, n, d, max(1, nlist // 4), a.sigma, n + len(a.corpus))
    q = q[:a.nq]
    n_train = min(n, 64 * nlist)

    built = {}
    for name, train in (("flat", pkg.ivf_ann.FaissIvfFlat.train), ("sq8", sq.FaissIvfSq8.train)):
        t0 = time.perf_counter()
        ix = train(m, nlist, x[:n_train], niter=a.niter, seed=1)
        t1 = time.perf_counter()
        ix.add(x)
        built[name] = (ix, round(t1 - t0, 3), round(time.perf_counter() - t1, 3))
    flat, sq8 = built["flat"][0], built["sq8"][0]
    assert flat.centroids().tobytes() == sq8.centroids().tobytes(), "the two indexes must share their centroids"
    sizes = flat.list_sizes()
    assert np.array_equal(sizes, sq8.list_sizes())
    slots = int(((sizes + 31) // 32).sum()) * 32
    dense = pkg.dense_ann.BruteForceIndex.build(m, x)
    del x

    by_k = {}
    for k in [int(s) for s in a.ks.split(",")]:
        t_ids, _, t_cnt = dense.search(q, k)
        stats = {"flat": [], "sq8": []}
        answers = {}
        for rep in range(-1, a.reps):  # rep -1 warms both up
            for name, ix in (("flat", flat), ("sq8", sq8)):
                t0 = time.perf_counter()
                answers[name] = ix.search(q, k, a.nprobe)
                st = ix.last_stats()
                st["call_ms"] = (time.perf_counter() - t0) * 1e3
                if rep >= 0:
                    stats[name].append(st)
            assert flat.last_probes().tobytes() == sq8.last_probes().tobytes(), "the two indexes must probe the same cells"
        f_ids, _, f_cnt = answers["flat"]
        s_ids, _, s_cnt = answers["sq8"]
        by_k[str(k)] = {
            **{name: {**{f: spread([s[f] for s in stats[name]]) for f in ("coarse_ms", "scan_ms", "select_ms", "call_ms")},
                      "rows_scanned": stats[name][0]["rows_scanned"], "rounds": max(s["rounds"] for s in stats[name])}
               for name in ("flat", "sq8")},
            "scan_ms_sq8_over_flat": round(float(np.median([s["scan_ms"] for s in stats["sq8"]])
                                                 / max(np.median([s["scan_ms"] for s in stats["flat"]]), 1e-9)), 4),
            "recall_sq8_vs_flat": recall(s_ids, s_cnt, f_ids, f_cnt),
            "recall_flat_vs_exhaustive": recall(f_ids, f_cnt, t_ids, t_cnt),
            "recall_sq8_vs_exhaustive": recall(s_ids, s_cnt, t_ids, t_cnt),
        }
    print(json.dumps({
        "corpus": a.corpus, "metric": a.metric, "n": n, "d": d, "nlist": nlist, "n_train": n_train, "niter": a.niter, "sigma": a.sigma,
        "nq": len(q), "nprobe": a.nprobe, "reps": a.reps,
        "train_s": {name: built[name][1] for name in built}, "add_s": {name: built[name][2] for name in built},
        "list_size_min": int(sizes.min()), "list_size_max": int(sizes.max()),
        "list_bytes_per_row": {"flat": round(slots * (2 * d + 8) / n, 2), "sq8": round(slots * (d + 8) / n, 2)},
        "by_k": by_k}), flush=True)
    flat.close()
    sq8.close()
    dense.close()


if __name__ == "__main__":
    main()
