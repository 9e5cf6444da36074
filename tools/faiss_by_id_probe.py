"""By-id queries on the inverted-file family and a shard set against the host composition they replace.

Shape: d = 256, 1M rows, `OPQ64,IVF4096,PQ64` and `IVF4096,Flat`, nprobe 16, k 10 and 200, n_seeds in {1, 64, 1024} (about
10 % absent, some repeated), and one ShardSet of 24 small shards.  Timed, alternating in one process after a warm-up, each
leg ending synchronised (both return host arrays), at least seven runs each:
  (a) FaissQueryableById.batch_arrays (seed ids up, flattened triples down)
  (b) the host composition over the unchanged plain searches: EmbeddingStore.get (device -> host), the plain search of the
      fetched rows (host -> device), flatten on the host
Before anything is timed the two answers are compared bit for bit.  The baseline is (b); the code under test is never its
own baseline, and no threshold is set: one JSON line per shape with wall time (median, min..max), the three HIP-event
times and the bus bytes up and down of both legs."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402


def host_composition(store, search, seeds):
    rows, found = store.get(seeds)                                # n_seeds x d floats come down ...
    counts = np.full(len(seeds), -1, np.int32)
    if not found.any():
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32), counts
    ids, dist, cnt = search(rows[found])                          # ... and n_found x d go up again
    keep = np.arange(ids.shape[1])[None, :] < cnt[:, None]
    counts[found] = cnt
    return np.repeat(seeds[found], cnt), ids[keep], dist[keep], counts


def spread(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), max_ms=float(a[-1]))


def run(name, q, by_id, host, seeds, reps, extra):
    got, want = by_id(), host()
    for g, w in zip(got, want):                                   # parity first: equal seeds, ids, distance bits, counts
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), name
    for _ in range(3):
        by_id(); host()
    ta, tb, phases = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter(); by_id(); ta.append((time.perf_counter() - t0) * 1e3)
        phases.append(q.last_stats())
        t0 = time.perf_counter(); host(); tb.append((time.perf_counter() - t0) * 1e3)
    st = phases[-1]
    a, b = spread(ta), spread(tb)
    overlap = a["min_ms"] <= b["max_ms"] and b["min_ms"] <= a["max_ms"]
    line = dict(probe="faiss_by_id", index=name, seeds=len(seeds), found=st["found"], absent=st["absent"], triples=int(len(got[0])),
                parity="bit-identical", repetitions=reps, by_id=a, host_composition=b,
                verdict="no speed claim (the spreads overlap)" if overlap else "the spreads do not overlap",
                resolve_gather_ms=float(np.median([p["resolve_gather_ms"] for p in phases])),
                search_ms=float(np.median([p["search_ms"] for p in phases])),
                flatten_ms=float(np.median([p["flatten_ms"] for p in phases])),
                h2d_bytes=st["h2d_bytes"], d2h_bytes=st["d2h_bytes"], d2h_result_bytes=st["d2h_result_bytes"],
                host_composition_h2d_bytes=8 * len(seeds) + 4 * int(st["found"]) * extra["dim"],
                host_composition_d2h_bytes=len(seeds) * (4 * extra["dim"] + 1) + int(st["found"]) * (12 * extra["k"] + 4), **extra)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--ks", default="10,200")
    ap.add_argument("--seeds", default="1,64,1024")
    ap.add_argument("--shards", type=int, default=24)
    ap.add_argument("--shard-rows", type=int, default=20_000)
    ap.add_argument("--shard-nlist", type=int, default=64)
    ap.add_argument("--niter", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", choices=["opq", "flat", "set", "all"], default="all")
    a = ap.parse_args()
    assert a.reps >= 7, "at least seven runs of each leg"
    pkg = load_package()
    fb = importlib.import_module(pkg.__name__ + ".faiss_by_id")
    m = pkg.dense_ann.DistanceMetric.L2
    P = pkg.ivf_ann.FaissParams
    rng = np.random.default_rng(0)
    centres = rng.standard_normal((1024, a.dim), dtype=np.float32) * 2
    x = np.empty((a.vectors, a.dim), np.float32)
    for r0 in range(0, a.vectors, 1 << 18):
        n = min(1 << 18, a.vectors - r0)
        x[r0:r0 + n] = centres[rng.integers(0, 1024, n)] + rng.standard_normal((n, a.dim), dtype=np.float32)
    keys = 1_000_000_000 + 3 * rng.permutation(a.vectors).astype(np.int64)
    store = pkg.ann_by_id.EmbeddingStore.build(keys, x)
    print(f"store of {a.vectors} keys built", file=sys.stderr, flush=True)
    train = x[: max(a.vectors // 10, min(a.vectors, 64 * a.nlist))]

    def seed_list(n):
        s = keys[rng.integers(0, a.vectors, n)]
        s[rng.random(n) < 0.10] += 1
        if n >= 8:
            s[4:8] = s[0:4]
        return np.ascontiguousarray(s)

    def legs(name, index, search, extra):
        q = fb.FaissQueryableById(store, index, m)
        for k in (int(v) for v in a.ks.split(",")):
            for n in (int(v) for v in a.seeds.split(",")):
                seeds = seed_list(n)
                run(name, q, lambda: q.batch_arrays(seeds, k, P(nprobe=a.nprobe)), lambda: host_composition(store, lambda r: search(r, k), seeds),
                    seeds, a.reps, dict(extra, k=k, nprobe=a.nprobe, vectors=a.vectors, dim=a.dim))

    if a.only in ("flat", "all"):
        t0 = time.time()
        ix = pkg.ivf_ann.FaissIvfFlat.train(m, a.nlist, train, niter=a.niter)
        ix.add(x, keys)
        print(f"IVF{a.nlist},Flat built in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
        legs(f"IVF{a.nlist},Flat", ix, lambda r, k: ix.search(r, k, a.nprobe), {})
        ix.close()
    if a.only in ("opq", "all"):
        t0 = time.time()
        ix = pkg.opq_ann.FaissOpqIvfPq.train(m, a.nlist, a.m, a.dim, train, niter=a.niter)
        ix.add(x, keys)
        print(f"OPQ{a.m},IVF{a.nlist},PQ{a.m} built in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
        legs(f"OPQ{a.m},IVF{a.nlist},PQ{a.m}", ix, lambda r, k: ix.search(r, k, a.nprobe), {})
        ix.close()
    if a.only in ("set", "all"):
        t0 = time.time()
        members = []
        for s in range(a.shards):
            r0 = s * a.shard_rows
            mb = pkg.ivf_ann.FaissIvfFlat.train(m, a.shard_nlist, x[r0:r0 + a.shard_rows], niter=a.niter)
            mb.add(x[r0:r0 + a.shard_rows], keys[r0:r0 + a.shard_rows])
            members.append(mb)
        ss = pkg.shard_set.ShardSet.create(m, a.dim)
        ss.set_members(members)
        print(f"{a.shards} shards of {a.shard_rows} rows built in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
        legs(f"ShardSet of {a.shards} x IVF{a.shard_nlist},Flat", ss, lambda r, k: ss.search(r, k, a.nprobe),
             dict(shards=a.shards, shard_rows=a.shard_rows))
        ss.close()
        for mb in members:
            mb.close()
    store.close()


if __name__ == "__main__":
    main()
