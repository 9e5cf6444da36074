"""What the OPQ pre-transform costs and finds (include/opq_ann.h), against the exhaustive index and against plain IVF-PQ
with the same nlist, M, niter and seed on the same rows in the same process.  One JSON line:
  train_s and its split   opq_index_train on the first n_train rows: transform_ms, pq_ms, correlation_ms, procrustes_ms (the
                          host's Jacobi), inner_ms (the IVF-PQ training on the transformed rows); training_err first / last
  add_s                   opq_index_add of all rows
  qps, ms, transform_ms   opq_search (best of --reps batches of nq queries) with the transform kernel's own milliseconds,
                          beside coarse / scan / select
  recall, pq_recall       recall@k against dann_search, for the OPQ index and for plain IVF-PQ; pq_train_s / pq_add_s / pq_qps
--default-shape takes nlist, M and d_out from the reference's default factory string for (n, dim).

Run each setting under its own time limit, e.g.
  timeout -k 10 900 python tools/opq_probe.py --n 100000 --dim 256 --default-shape > profiles/opq_probe_100k_default.json"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ivf_probe import best_time, corpus  # noqa: E402
from ivfpq_probe import recall_of  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", default="clustered", choices=["clustered", "iid"])
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--d-out", type=int, default=0)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--M", type=int, default=32)
    ap.add_argument("--default-shape", action="store_true")
    ap.add_argument("--n-train", type=int, default=0)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--niter-opq", type=int, default=0)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--metric", default="L2")
    a = ap.parse_args()
    pkg = load_package()
    oq = pkg.opq_ann
    m = getattr(pkg.dense_ann.DistanceMetric, a.metric)
    n, d = a.n, a.dim
    nlist, M, d_out = a.nlist, a.M, a.d_out or d
    if a.default_shape:
        spec = oq.index_factory(d, oq.default_factory_string(n, d), m)
        nlist, M, d_out = spec.nlist, spec.M, spec.d_out
    x, q = corpus(a.corpus, n, d, max(1, nlist // 4), a.sigma, n + len(a.corpus))
    q = q[:a.nq]
    n_train = min(n, a.n_train or 64 * nlist)
    k, nprobe = a.k, a.nprobe

    dense = pkg.dense_ann.BruteForceIndex.build(m, x)
    dense.search(q, k)
    dense_s, truth = best_time(lambda: dense.search(q, k), a.reps)
    dense.close()

    t0 = time.perf_counter()
    ix = oq.FaissOpqIvfPq.train(m, nlist, M, d_out, x[:n_train], niter=a.niter, niter_opq=a.niter_opq, seed=1)
    train_s = time.perf_counter() - t0
    tr, err = ix.training_stats(), ix.training_errors()
    t0 = time.perf_counter()
    ix.add(x)
    add_s = time.perf_counter() - t0
    ix.search(q, k, nprobe)  # warm-up
    s, (ids, _, cnt) = best_time(lambda: ix.search(q, k, nprobe), a.reps)
    st = ix.last_stats()
    line = {"corpus": a.corpus, "metric": a.metric, "n": n, "d_in": d, "d_out": d_out, "nlist": nlist, "M": M, "n_train": n_train,
            "niter": a.niter, "niter_opq": len(err), "nq": len(q), "k": k, "nprobe": nprobe, "train_s": round(train_s, 3),
            "training_err_first": float(err[0]), "training_err_last": float(err[-1]), "add_s": round(add_s, 3),
            "qps": round(len(q) / s, 1), "ms": round(s * 1e3, 3), "dense_qps": round(len(q) / dense_s, 1),
            "rows_scanned": st["rows_scanned"], "rounds": st["rounds"],
            "recall": round(recall_of(ids, cnt, truth[0], truth[2]), 4)}
    line.update({key: round(v, 3) for key, v in tr.items()})
    line.update({key: round(st[key], 3) for key in ("transform_ms", "coarse_ms", "scan_ms", "select_ms")})
    ix.close()

    # plain IVF-PQ needs M to divide the dimension itself: at the reference's default shape (256 / 48) it cannot be built,
    # which is the reason the reference projects to 240 first
    if d % M == 0:
        t0 = time.perf_counter()
        pq = pkg.ivfpq_ann.FaissIvfPq.train(m, nlist, M, x[:n_train], niter=a.niter, seed=1)
        line["pq_train_s"] = round(time.perf_counter() - t0, 3)
        t0 = time.perf_counter()
        pq.add(x)
        line["pq_add_s"] = round(time.perf_counter() - t0, 3)
        pq.search(q, k, nprobe)
        s, (ids, _, cnt) = best_time(lambda: pq.search(q, k, nprobe), a.reps)
        line["pq_qps"] = round(len(q) / s, 1)
        line["pq_recall"] = round(recall_of(ids, cnt, truth[0], truth[2]), 4)
        pq.close()
    else:
        line["pq_recall"] = None
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
