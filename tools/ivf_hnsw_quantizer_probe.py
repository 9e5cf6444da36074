"""The two coarse quantizers of an IVF index side by side (include/ivf_hnsw_quantizer.h): one IVF-Flat index over --nlist
centroids of dimension --dim serves both, the exhaustive search (detached) and the HNSW graph (attached).  JSON lines:
  {"what": "build"}    the device build of the graph over the centroids: seconds, max_m, ef_construction
  {"what": "coarse"}   coarse_ms (HIP events 0 -> 1 of ivf_last_stats: query preparation, the coarse search, the probe
                       inversion) of each quantizer per nq, the best of --reps searches, at --nprobe and the given quantizer_ef
  {"what": "add"}      seconds to add --n-add rows through each quantizer (a fresh index each), and the same per 1M rows
  {"what": "recall"}   the share of the exhaustive probes that the walk's probes hold, per (quantizer_ef, nprobe), with the
                       walks' distance evaluations per query and the probes they did not find
The centroids are rows of the clustered corpus of tools/ivf_probe.py (no k-means: the probe measures the coarse step, not the
cells).  No number here is a target: the default quantizer stays the exhaustive one.

Run each nlist under its own time limit, e.g.
  timeout -k 10 900 python tools/ivf_hnsw_quantizer_probe.py --nlist 4096 > profiles/ivf_hnsw_quantizer_probe_4096.jsonl
  timeout -k 10 900 python tools/ivf_hnsw_quantizer_probe.py --nlist 65536 > profiles/ivf_hnsw_quantizer_probe_65536.jsonl"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ivf_probe import corpus  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--max-m", type=int, default=32)
    ap.add_argument("--ef-construction", type=int, default=40)
    ap.add_argument("--nqs", default="1,64,1024")
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--efs", default="16,64,256")
    ap.add_argument("--nprobes", default="1,16,128")
    ap.add_argument("--n-add", type=int, default=262144)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--metric", default="L2")
    a = ap.parse_args()
    pkg = load_package()
    hq = importlib.import_module(pkg.__name__ + ".hnsw_quantizer")
    m = getattr(pkg.dense_ann.DistanceMetric, a.metric)
    nlist, d = a.nlist, a.dim
    x, q = corpus("clustered", max(a.n_add, nlist), d, max(nlist // 4, 1), a.sigma, nlist)
    cent = x[np.random.default_rng(1).choice(len(x), nlist, replace=False)]
    base = {"metric": a.metric, "nlist": nlist, "d": d, "max_m": a.max_m, "ef_construction": a.ef_construction}

    def line(what, **fields):
        print(json.dumps({"what": what, **base, **fields}), flush=True)

    ix = pkg.ivf_ann.FaissIvfFlat.load(m, cent)
    t0 = time.perf_counter()
    hq.attach(ix, max_m=a.max_m, ef_construction=a.ef_construction)
    line("build", build_s=round(time.perf_counter() - t0, 3), build_stats=list(hq.quantizer(ix).build_stats()))
    graph = hq.quantizer(ix).graph()

    def coarse_ms(nq, nprobe):
        ix.search(q[:nq], 10, nprobe)  # warm-up
        best = None
        for _ in range(a.reps):
            ix.search(q[:nq], 10, nprobe)
            ms = ix.last_stats()["coarse_ms"]
            best = ms if best is None else min(best, ms)
        return round(best, 4)

    efs = [int(s) for s in a.efs.split(",")]
    for nq in (int(s) for s in a.nqs.split(",")):
        fields = {"nq": nq, "nprobe": a.nprobe}
        hq.detach(ix)
        fields["exhaustive_coarse_ms"] = coarse_ms(nq, a.nprobe)
        hq.attach(ix, max_m=a.max_m, graph=graph)
        for ef in efs:
            hq.set_quantizer_ef(ix, ef)
            fields[f"hnsw_ef{ef}_coarse_ms"] = coarse_ms(nq, a.nprobe)
        line("coarse", **fields)

    nq = min(1024, len(q))
    for nprobe in (int(s) for s in a.nprobes.split(",")):
        hq.detach(ix)
        ix.search(q[:nq], 10, nprobe)
        exact = ix.last_probes()
        hq.attach(ix, max_m=a.max_m, graph=graph)
        for ef in efs:
            hq.set_quantizer_ef(ix, ef)
            ix.search(q[:nq], 10, nprobe)
            walk, st = ix.last_probes(), hq.last_quantizer_stats(ix)
            hits = sum(len(np.intersect1d(w[w >= 0], e)) for w, e in zip(walk, exact))
            line("recall", nq=nq, nprobe=int(exact.shape[1]), quantizer_ef=ef, probe_recall=round(hits / exact.size, 4),
                 distance_evals_per_query=round(st["distance_evals"] / nq, 1), missing_probes=st["missing_probes"])
    ix.close()

    fields = {"n_add": a.n_add, "quantizer_ef": 16}
    for name in ("exhaustive", "hnsw"):
        ix = pkg.ivf_ann.FaissIvfFlat.load(m, cent)
        if name == "hnsw":
            hq.attach(ix, max_m=a.max_m, graph=graph)
        t0 = time.perf_counter()
        ix.add(x[:a.n_add])
        s = time.perf_counter() - t0
        fields[f"{name}_add_s"] = round(s, 3)
        fields[f"{name}_add_s_per_1M"] = round(s * 1e6 / a.n_add, 3)
        ix.close()
    line("add", **fields)


if __name__ == "__main__":
    main()
