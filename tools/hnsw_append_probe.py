"""What appending costs (hnsw_index_append / dann_index_append), measured in one process per corpus.  One JSON line per
configuration:
  append      per base n and append size B: appended rows/s and p50 / p99 call latency (every call ends with a device
              synchronise: hnsw_index_append returns when its rounds are done)
  grow        0.5 n -> n by appends of 4096 against the one-shot device build: build(n) - build(0.5 n) is the time the
              one-shot build spends on the rounds that insert rows 0.5 n .. n (the same rounds an append runs, from the same
              schedule position)
  search      k=10/ef=100 and k=200/ef=800 queries/s on the base, and after growing it by 10 %
  recall      recall@10 (ef=100) of the grown index and of the one-shot build of the same rows, against brute force
  dense       BruteForceIndex.append rows/s for B = 4096 into a synthetic n x 256 index
Corpora: i.i.d. N(0,1) and a mixture of 1000 Gaussians, d = 256, maxM = 16, efConstruction = 200, Cosine."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402


def corpus(kind, n, d, rng, centres=None):
    """i.i.d. N(0,1) rows, or a mixture of Gaussians around `centres` (1000 of them, drawn from rng when not given)."""
    if kind == "iid":
        return rng.standard_normal((n, d), dtype=np.float32)
    if centres is None:
        centres = np.random.default_rng(12345).standard_normal((1000, d), dtype=np.float32)
    out = np.empty((n, d), np.float32)
    for s in range(0, n, 1 << 20):
        e = min(n, s + (1 << 20))
        out[s:e] = centres[rng.integers(0, 1000, e - s)] + 0.6 * rng.standard_normal((e - s, d), dtype=np.float32)
    return out


def emit(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default="1000000,10000000", help="base sizes n")
    ap.add_argument("--corpora", default="iid,clustered")
    ap.add_argument("--sizes", default="1,64,4096,65536", help="append sizes B")
    ap.add_argument("--calls", default="200,100,20,3", help="appends timed per B")
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--dense-n", type=int, default=50_000_000, help="0 = skip the dense line")
    ap.add_argument("--skip-grow", action="store_true")
    ap.add_argument("--append-only", action="store_true", help="only the append lines (the shape a kernel / memory-copy trace wants)")
    a = ap.parse_args()
    pkg = load_package()
    Hnsw, m = pkg.hnsw_ann.Hnsw, pkg.dense_ann.DistanceMetric.Cosine
    d, M, efc = a.dim, 16, 200
    sizes, calls = [int(s) for s in a.sizes.split(",")], [int(s) for s in a.calls.split(",")]
    for kind in a.corpora.split(","):
        for n in [int(s) for s in a.base.split(",")]:
            rng = np.random.default_rng(n + len(kind))
            extra = sum(b * c for b, c in zip(sizes, calls))
            grow = n // 10
            x = corpus(kind, n + max(extra, grow), d, rng)
            q = corpus(kind, a.queries, d, np.random.default_rng(7))  # (clustered: around the corpus's centres)
            t = time.perf_counter()
            ix = Hnsw.build(m, x[:n], max_m=M, ef_construction=efc, seed=1, gpu=True)
            t_build = time.perf_counter() - t

            def qps(index, k, ef):
                index.search(q, k, ef)
                t0 = time.perf_counter()
                index.search(q, k, ef)
                return a.queries / (time.perf_counter() - t0)

            base_qps = {f"{k}/{ef}": qps(ix, k, ef) for k, ef in ((10, 100), (200, 800))}
            # ---- append cost by B ----
            at = n
            for b, c in zip(sizes, calls):
                lat = []
                for _ in range(c):
                    t0 = time.perf_counter()
                    ix.append(x[at:at + b], ef_construction=efc, seed=1)
                    lat.append(time.perf_counter() - t0)
                    at += b
                lat = np.array(lat)
                emit(what="append", corpus=kind, base_n=n, B=b, calls=c, rows_per_s=b * c / float(lat.sum()),
                     p50_ms=1e3 * float(np.percentile(lat, 50)), p99_ms=1e3 * float(np.percentile(lat, 99)), rounds_last=ix.build_stats()[0],
                     n_after=ix.n, build_s=t_build)
            ix.close()
            if a.append_only:
                continue
            # ---- search before / after 10 % growth, recall of the grown index vs the one-shot build ----
            ix = Hnsw.build(m, x[:n], max_m=M, ef_construction=efc, seed=1, gpu=True)
            t0 = time.perf_counter()
            for s in range(n, n + grow, 4096):
                ix.append(x[s:min(n + grow, s + 4096)], ef_construction=efc, seed=1)
            t_grow10 = time.perf_counter() - t0
            grown_qps = {f"{k}/{ef}": qps(ix, k, ef) for k, ef in ((10, 100), (200, 800))}
            one = Hnsw.build(m, x[:n + grow], max_m=M, ef_construction=efc, seed=1, gpu=True)
            bf = pkg.dense_ann.BruteForceIndex.build(m, x[:n + grow])
            t_ids, _, _ = bf.search(q[:1024], 10)
            bf.close()

            def recall(index):
                ids, _, cnt = index.search(q[:1024], 10, 100)
                return float(np.mean([len(set(ids[i, :cnt[i]]) & set(t_ids[i])) / 10 for i in range(1024)]))

            emit(what="search", corpus=kind, base_n=n, grown_n=n + grow, qps_before=base_qps, qps_after_growth=grown_qps,
                 recall10_grown=recall(ix), recall10_one_shot=recall(one), grow_by_4096_s=t_grow10)
            ix.close(); one.close()
            # ---- 0.5 n -> n by appends of 4096 vs the same rounds of a one-shot build ----
            if not a.skip_grow:
                h = n // 2
                t0 = time.perf_counter()
                half = Hnsw.build(m, x[:h], max_m=M, ef_construction=efc, seed=1, gpu=True)
                t_half = time.perf_counter() - t0
                t0 = time.perf_counter()
                full = Hnsw.build(m, x[:n], max_m=M, ef_construction=efc, seed=1, gpu=True)
                t_full = time.perf_counter() - t0
                full.close()
                t0 = time.perf_counter()
                for s in range(h, n, 4096):
                    half.append(x[s:min(n, s + 4096)], ef_construction=efc, seed=1)
                t_app = time.perf_counter() - t0
                half.close()
                emit(what="grow", corpus=kind, from_n=h, to_n=n, appends_of=4096, append_s=t_app, one_shot_build_s=t_full,
                     half_build_s=t_half, one_shot_same_rounds_s=t_full - t_half, ratio=t_app / max(1e-9, t_full - t_half))
            del x
    if a.dense_n > 0:
        B = pkg.dense_ann.BruteForceIndex
        ix = B.synthetic(pkg.dense_ann.DistanceMetric.L2, a.dense_n, 256, seed=1)
        rows = np.random.default_rng(3).standard_normal((4096 * 20, 256), dtype=np.float32)
        lat = []
        for c in range(20):
            t0 = time.perf_counter()
            ix.append(rows[c * 4096:(c + 1) * 4096])
            lat.append(time.perf_counter() - t0)
        lat = np.array(lat)
        emit(what="dense_append", base_n=a.dense_n, d=256, B=4096, calls=20, rows_per_s=4096 * 20 / float(lat.sum()),
             p50_ms=1e3 * float(np.percentile(lat, 50)), p99_ms=1e3 * float(np.percentile(lat, 99)))
        ix.close()


if __name__ == "__main__":
    main()
