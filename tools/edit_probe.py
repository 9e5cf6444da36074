"""The EditDistance index (include/edit_ann.h) at size: --n strings of length --min-len..--max-len over a --symbols-symbol
alphabet, --nq queries from the same distribution, at every k of --ks.  One JSON line per k:
  distance_ms, select_ms   HIP events of the last of --reps searches (edit_last_timing), and the best of the reps
  wall_ms                  the best search call as Python sees it (uploads of the queries and downloads of the answers included)
  pairs_per_s, cell_updates_per_s   from edit_last_stats over the best distance_ms + select_ms
  host_*                   edit_pair_distances_host on --host-threads threads over --host-queries of the queries against
                           every row; host_scaled_ms is that time scaled by nq / host_queries -- a scaled figure, never a
                           measured run of all the queries
  first_search_ms          the first search, which also lays the rows on the device
The lines go to standard output and, with --out, to that file as well.  No number here is a target.

Run under a time limit of its own, e.g.
  timeout -k 10 600 python tools/edit_probe.py --out profiles/edit_probe_1m.jsonl"""
import argparse
import importlib
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402


def strings(rng, n, lo, hi, symbols):
    lens = rng.integers(lo, hi + 1, n)
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    return offsets, rng.integers(1, symbols + 1, int(offsets[-1])).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--min-len", type=int, default=4)
    ap.add_argument("--max-len", type=int, default=32)
    ap.add_argument("--symbols", type=int, default=36)
    ap.add_argument("--ks", default="10,200")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-queries", type=int, default=16)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = load_package()
    ed = importlib.import_module(pkg.__name__ + ".edit_distance")
    rng = np.random.default_rng(1)
    rows = strings(rng, a.n, a.min_len, a.max_len, a.symbols)
    queries = strings(rng, a.nq, a.min_len, a.max_len, a.symbols)
    base = {"n": a.n, "nq": a.nq, "lengths": [a.min_len, a.max_len], "symbols": a.symbols}
    out = open(a.out, "w") if a.out else None

    t0 = time.perf_counter()
    index = ed.EditBruteForceIndex(rows)
    build_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    index.search(queries, 1)
    first_ms = (time.perf_counter() - t0) * 1e3

    # the host baseline: host_queries queries against every row, one query per task
    hq = min(a.host_queries, a.nq)
    q_off, q_chars = queries

    def one(q):
        s = q_chars[q_off[q]:q_off[q + 1]]
        a_off = np.arange(a.n + 1, dtype=np.int64) * len(s)
        return ed.pair_distances(a_off, np.tile(s, a.n), rows[0], rows[1])

    t0 = time.perf_counter()
    with ThreadPoolExecutor(a.host_threads) as pool:
        host = list(pool.map(one, range(hq)))
    host_ms = (time.perf_counter() - t0) * 1e3

    for k in [int(x) for x in a.ks.split(",")]:
        runs = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            dist, ids, counts = index.search(queries, k)
            wall = (time.perf_counter() - t0) * 1e3
            runs.append((index.last_timing(), wall))
        t = runs[-1][0]
        best = (min((r[0] for r in runs), key=lambda x: x["distance_ms"] + x["select_ms"]), min(r[1] for r in runs))
        stats = index.last_stats()
        device_s = (best[0]["distance_ms"] + best[0]["select_ms"]) / 1e3
        # the device against the host on the queries the host scored: the k nearest distances must agree
        agree = all(np.array_equal(np.sort(host[q], kind="stable")[:k], dist[q, :counts[q]]) for q in range(hq))
        line = {"what": "edit_probe", **base, "k": k, "distance_ms": round(best[0]["distance_ms"], 3), "select_ms": round(best[0]["select_ms"], 3),
                "last_distance_ms": round(t["distance_ms"], 3), "last_select_ms": round(t["select_ms"], 3), "wall_ms": round(best[1], 3),
                "pairs": stats["pairs"], "cell_updates": stats["cell_updates"], "pairs_per_s": round(stats["pairs"] / device_s),
                "cell_updates_per_s": round(stats["cell_updates"] / device_s), "reps": a.reps, "build_s": round(build_s, 3),
                "first_search_ms": round(first_ms, 3), "host_queries": hq, "host_threads": a.host_threads, "host_ms": round(host_ms, 3),
                "host_scaled_ms": round(host_ms * a.nq / hq, 3), "host_scaled_label": f"{hq} queries measured, scaled to {a.nq}",
                "host_agrees_on_distances": bool(agree)}
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()
    index.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
