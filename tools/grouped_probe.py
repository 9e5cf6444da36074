"""What the grouped index costs (include/grouped_ann.h), against the composition the reference performs on the same rows in
the same process: one dann_index_t per group and one dann_search per distinct key of the batch.  One process per corpus;
one JSON line per (key distribution, k):
  grouped_qps       queries/s of gann_search (best of --reps batches of nq queries), and its work-list / scan / select
                    milliseconds, tiles, work items, rounds, rows scanned
  bytes_read        what the scan's workgroups read in round 0: per group, tiles x 32-row blocks of its list, plus the first
                    segment once more per tile of a group above 8192 rows (the sample pass); fallback rounds re-read part
                    of it and are not counted.  hbm_frac = bytes_read / scan time / 8 TB/s: tiles of one segment run
                    together and share the caches, so it is a rate of requested bytes and may exceed 1
  loop_qps          queries/s of the per-group loop; loop_searches = distinct keys of the batch = its dann_search calls
  *_device_bytes    device memory held after the build (hipMemGetInfo before and after)
  agree             share of queries whose id lists are equal in the two answers
Corpus: N(0,1) rows of dimension --dim in --groups groups; group g holds max(--min-rows, --max-rows / (g + 1)^2) rows.
Query keys: `uniform` over the groups, or `proportional` to group size.

Run under a time limit of its own, e.g.
  timeout -k 10 900 python tools/grouped_probe.py > profiles/grouped_probe_d256_g256.jsonl"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X
CAP = 8192


def best_time(fn, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, r


def device_free():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    if hip.hipMemGetInfo(C.byref(free), C.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return free.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--groups", type=int, default=256)
    ap.add_argument("--max-rows", type=int, default=1 << 20)
    ap.add_argument("--min-rows", type=int, default=24)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--ks", default="10,200")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--metric", default="L2")
    a = ap.parse_args()
    pkg = load_package()
    m = getattr(pkg.dense_ann.DistanceMetric, a.metric)
    d, ng = a.dim, a.groups
    sizes = np.maximum(a.min_rows, a.max_rows // (np.arange(ng, dtype=np.int64) + 1) ** 2)
    start = np.concatenate([[0], np.cumsum(sizes)])
    n = int(start[-1])
    rng = np.random.default_rng(n + ng)
    x = np.empty((n, d), np.float32)
    for s in range(0, n, 1 << 18):
        e = min(n, s + (1 << 18))
        x[s:e] = rng.standard_normal((e - s, d), dtype=np.float32)
    groups = np.repeat(np.arange(ng, dtype=np.int32), sizes)
    q = rng.standard_normal((a.nq, d), dtype=np.float32)
    batches = {"uniform": rng.integers(0, ng, a.nq).astype(np.int32),
               "proportional": rng.choice(ng, a.nq, p=sizes / sizes.sum()).astype(np.int32)}

    # the runtime's own first allocations (context, code objects) belong to neither side: a tiny index of each kind first
    pkg.grouped_ann.GroupedIndex.build_numbered(x[:64], None, groups[:64] * 0, ["0"], m).close()
    pkg.dense_ann.BruteForceIndex.build(m, x[:64]).close()
    free0 = device_free()
    t0 = time.perf_counter()
    gx = pkg.grouped_ann.GroupedIndex.build_numbered(x, None, groups, [str(g) for g in range(ng)], m)
    grouped_build_s = time.perf_counter() - t0
    free1 = device_free()
    t0 = time.perf_counter()
    ids = np.arange(n, dtype=np.int64)
    loop = [pkg.dense_ann.BruteForceIndex.build(m, x[start[g]:start[g + 1]], ids[start[g]:start[g + 1]]) for g in range(ng)]
    loop_build_s = time.perf_counter() - t0
    free2 = device_free()
    del x

    def loop_search(qg, k):
        out_ids = np.zeros((len(qg), k), np.int64)
        out_cnt = np.zeros(len(qg), np.int32)
        for g in np.unique(qg):
            sel = np.flatnonzero(qg == g)
            i, _, c = loop[g].search(q[sel], k)
            out_ids[sel], out_cnt[sel] = i, c
        return out_ids, out_cnt

    for name, qg in batches.items():
        for k in [int(s) for s in a.ks.split(",")]:
            gx.search_groups(q, qg, k)  # warm-up
            g_s, (g_ids, _, g_cnt) = best_time(lambda: gx.search_groups(q, qg, k), a.reps)
            st = gx.last_stats()
            loop_search(qg, k)  # warm-up
            l_s, (l_ids, l_cnt) = best_time(lambda: loop_search(qg, k), a.reps)
            per = np.bincount(qg, minlength=ng)
            tiles = (per + 31) // 32
            rows_read = int((tiles * ((sizes + 31) // 32) * 32).sum() + (tiles * (sizes > CAP) * st["segment_rows"]).sum())
            scan_s = max(st["scan_ms"], 1e-6) * 1e-3
            agree = float(np.mean([g_cnt[i] == l_cnt[i] and np.array_equal(g_ids[i, :g_cnt[i]], l_ids[i, :l_cnt[i]])
                                   for i in range(len(qg))]))
            print(json.dumps({
                "metric": a.metric, "n": n, "d": d, "groups": ng, "group_rows_min": int(sizes.min()),
                "group_rows_max": int(sizes.max()), "nq": len(qg), "keys": name, "distinct_keys": int(len(np.unique(qg))), "k": k,
                "grouped_qps": round(len(qg) / g_s, 1), "loop_qps": round(len(qg) / l_s, 1),
                "grouped_ms": round(g_s * 1e3, 3), "loop_ms": round(l_s * 1e3, 3), "loop_searches": int(len(np.unique(qg))),
                "worklist_ms": round(st["worklist_ms"], 3), "scan_ms": round(st["scan_ms"], 3), "select_ms": round(st["select_ms"], 3),
                "tiles": st["tiles"], "work_items": st["work_items"], "rounds": st["rounds"], "segment_rows": st["segment_rows"],
                "rows_scanned": st["rows_scanned"], "bytes_read": rows_read * d * 2,
                "hbm_frac": round(rows_read * d * 2 / scan_s / HBM_PEAK, 4),
                "grouped_build_s": round(grouped_build_s, 3), "loop_build_s": round(loop_build_s, 3),
                "grouped_device_bytes": free0 - free1, "loop_device_bytes": free1 - free2, "agree": round(agree, 4)}), flush=True)
    gx.close()
    for ix in loop:
        ix.close()


if __name__ == "__main__":
    main()
