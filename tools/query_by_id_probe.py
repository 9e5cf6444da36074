"""Query by id from the device embedding store against the host composition it replaces, at 1M x 256.

Setup: the i.i.d. HNSW index of tools/hnsw_bench.py (Cosine, maxM 16, efConstruction 200, device builder), a store of as many
keys, 4096 seeds (about 10 % absent, some repeated).  Timed, alternating in one process after a warm-up, each leg ending
synchronised (both return host arrays):
  (a) QueryableById.batchQueryWithDistanceById as arrays (seed ids up, flattened triples down)
  (b) the host composition: numpy gather of the seeds' rows, Hnsw.search / BruteForceIndex.search, flatten on the host
Before anything is timed the two answers are compared bit for bit.  One JSON line per configuration: median and spread
(min, max, interquartile range) of each leg over the repetitions, the phases' HIP-event times and the bus byte counters."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402


def host_composition(search, row_of_key, rows, seeds):
    r = row_of_key(seeds)
    found = r >= 0
    ids, dist, cnt = search(rows[r[found]])                      # numpy gather: n_found x d floats cross the bus
    k = ids.shape[1]
    keep = np.arange(k)[None, :] < cnt[:, None]
    counts = np.full(len(seeds), -1, np.int32)
    counts[found] = cnt
    return np.repeat(seeds[found], cnt), ids[keep], dist[keep], counts


def spread(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), max_ms=float(a[-1]),
                iqr_ms=float(np.percentile(a, 75) - np.percentile(a, 25)))


def run(name, q, by_id, host, seeds, reps, extra):
    got, want = by_id(), host()
    for g, w in zip(got, want):                                   # parity first: equal seeds, ids, distance bits, counts
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint32 if g.dtype == np.float32 else g.dtype),
                                                     w.view(np.uint32 if w.dtype == np.float32 else w.dtype)), name
    for _ in range(3):
        by_id(); host()
    ta, tb, phases = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter(); by_id(); ta.append((time.perf_counter() - t0) * 1e3)
        phases.append(q.last_stats())
        t0 = time.perf_counter(); host(); tb.append((time.perf_counter() - t0) * 1e3)
    st = phases[-1]
    line = dict(probe="query_by_id", index=name, seeds=len(seeds), found=st["found"], absent=st["absent"], triples=int(len(got[0])),
                parity="bit-identical", repetitions=reps, by_id=spread(ta), host_composition=spread(tb),
                resolve_gather_ms=float(np.median([p["resolve_gather_ms"] for p in phases])),
                search_ms=float(np.median([p["search_ms"] for p in phases])),
                flatten_ms=float(np.median([p["flatten_ms"] for p in phases])),
                h2d_bytes=st["h2d_bytes"], d2h_bytes=st["d2h_bytes"], d2h_result_bytes=st["d2h_result_bytes"], **extra)
    line["host_composition_h2d_bytes"] = int(st["found"]) * extra["dim"] * 4
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--store-keys", type=int, default=1_000_000)
    ap.add_argument("--seeds", type=int, default=4096)
    ap.add_argument("--configs", default="10:100,200:800")
    ap.add_argument("--dense-k", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["hnsw", "dense", "both"], default="both")
    ap.add_argument("--by-id-only", action="store_true", help="run leg (a) alone, `reps` times (for a kernel trace)")
    a = ap.parse_args()
    pkg = load_package()
    m = pkg.dense_ann.DistanceMetric.Cosine
    rng = np.random.default_rng(0)
    x = np.empty((a.vectors, a.dim), np.float32)
    for r0 in range(0, a.vectors, 1 << 20):
        x[r0:r0 + (1 << 20)] = rng.standard_normal((min(1 << 20, a.vectors - r0), a.dim), dtype=np.float32)
    keys = 1_000_000_000 + 3 * rng.permutation(a.store_keys).astype(np.int64)
    rows = rng.standard_normal((a.store_keys, a.dim), dtype=np.float32)
    seeds = keys[rng.integers(0, a.store_keys, a.seeds)]
    seeds[rng.random(a.seeds) < 0.10] += 1
    seeds[100:200] = seeds[0:100]
    order = np.argsort(keys)
    skeys = keys[order]

    def row_of_key(s):
        i = np.minimum(np.searchsorted(skeys, s), len(skeys) - 1)
        return np.where(skeys[i] == s, order[i], -1)

    store = pkg.EmbeddingStore.build(keys, rows)
    print(f"store of {a.store_keys} keys built", file=sys.stderr, flush=True)
    extra = dict(vectors=a.vectors, dim=a.dim, store_keys=a.store_keys)
    if a.only in ("hnsw", "both"):
        t0 = time.time()
        ix = pkg.hnsw_ann.Hnsw.build(m, x, max_m=16, ef_construction=200, seed=1, gpu=True)
        print(f"graph built in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
        q = pkg.QueryableById(store, ix)
        for cfg in a.configs.split(","):
            k, ef = (int(v) for v in cfg.split(":"))
            P = pkg.hnsw_ann.HnswParams(ef)
            by_id = lambda: q.batch_arrays(seeds, k, P)  # noqa: E731
            if a.by_id_only:
                for _ in range(a.reps):
                    by_id()
                continue
            run("hnsw", q, by_id, lambda: host_composition(lambda r: ix.search(r, k, ef), row_of_key, rows, seeds), seeds, a.reps,
                dict(extra, k=k, ef=ef))
        ix.close()
    if a.only in ("dense", "both"):
        bf = pkg.dense_ann.BruteForceIndex.build(m, x)
        q = pkg.QueryableById(store, bf)
        k = a.dense_k
        by_id = lambda: q.batch_arrays(seeds, k)  # noqa: E731
        if a.by_id_only:
            for _ in range(a.reps):
                by_id()
        else:
            run("brute_force", q, by_id, lambda: host_composition(lambda r: bf.search(r, k), row_of_key, rows, seeds), seeds, a.reps,
                dict(extra, k=k))
        bf.close()
    store.close()


if __name__ == "__main__":
    main()
