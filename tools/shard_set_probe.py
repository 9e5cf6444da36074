"""What serving S hourly shards as one index costs through the device-side set (include/shard_set.h, HourlyShardedIndex.search)
against the host composition it replaces (HourlyShardedIndex.search_composed: every shard's own search from host memory,
then dann_compose_shards), on the same loaded shards in the same process.  The baseline is the composition path; nothing is
compared against the new code's own output.

A case is (factory string, S, rows per shard, dim).  The shards of a case are S directories under one root, one hour apart,
written and loaded as the reference's job and server do (faiss_files.h).  Only the first shard is trained; the others take
its matrix, centroids and codebooks and add rows of their own -- training is not what is measured here.  `default` as the
factory string is the reference's default for that shard size and dimension (opq_ann.default_factory_string).

One JSON line per (case, k):
  set_ms, composed_ms        wall time of one call for nq queries, the median of --reps calls after --warmup calls of both
                             paths at this shape, the two paths alternating; each call ends with its answer on the host
  set_ms_min .. composed_ms_max   the spread of those calls
  search_ms, fold_ms         shardset_last_stats of the last set call: HIP-event time in the members' searches and in the folds
  set_h2d_bytes, set_d2h_bytes, set_d2h_result_bytes   the same call's bus bytes
  composed_h2d_bytes, composed_d2h_result_bytes        what the composition path moves, from its code: the queries once per
                             shard, and every shard's answer (12 nq k + 4 nq bytes); its control words are not counted
  same_answers               the two paths' answers are equal byte for byte

Run it under its own time limit, e.g.
  timeout -k 10 900 python tools/shard_set_probe.py > profiles/shard_set_probe_new.jsonl"""
import argparse
import datetime as dt
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ivf_probe import corpus  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

UTC = dt.timezone.utc


def build_shards(pkg, root, now, factory, S, rows, d, m, x, niter, niter_opq):
    """S hourly directories under root; returns the factory string used."""
    ff = pkg.faiss_files
    if factory == "default":
        factory = pkg.opq_ann.default_factory_string(rows, d)
    ids = np.arange(S * rows, dtype=np.int64)
    first = None
    for s in range(S):
        directory = os.path.join(root, (now - dt.timedelta(hours=s)).strftime("%Y/%m/%d/%H"))
        os.makedirs(os.path.dirname(directory), exist_ok=True)
        part, part_ids = x[s * rows:(s + 1) * rows], ids[s * rows:(s + 1) * rows]
        if first is None:
            ix = first = pkg.opq_ann.build_faiss_index(part, part_ids, 1.0, factory, m, niter=niter, niter_opq=niter_opq, seed=1)
        else:
            if isinstance(first, pkg.opq_ann.FaissOpqIvfPq):
                ix = pkg.opq_ann.FaissOpqIvfPq.load(m, first.matrix(), first.centroids(), first.codebooks())
            elif isinstance(first, pkg.ivfpq_ann.FaissIvfPq):
                ix = pkg.ivfpq_ann.FaissIvfPq.load(m, first.centroids(), first.codebooks())
            else:
                ix = pkg.ivf_ann.FaissIvfFlat.load(m, first.centroids())
            ix.add(part, part_ids)
        ff.write_index(ix, directory)
        if ix is not first:
            ix.close()
    first.close()
    return factory


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", default=None, metavar="FACTORY:S:ROWS:DIM",
                    help="may be repeated; default: default:24:20000:192, IVF256,Flat:24:20000:192 and default:4:20000:192")
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--ks", default="10,100,1000")
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--metric", default="Cosine")
    ap.add_argument("--niter", type=int, default=3)
    ap.add_argument("--niter-opq", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dir", default=None, help="where the directories are written (default: a temporary directory)")
    a = ap.parse_args()
    pkg = load_package()
    ff = pkg.faiss_files
    m = getattr(pkg.dense_ann.DistanceMetric, a.metric)
    now = dt.datetime(2024, 1, 2, 12, 30, tzinfo=UTC)
    cases = []
    for c in a.case or ["default:24:20000:192", "IVF256,Flat:24:20000:192", "default:4:20000:192"]:
        factory, S, rows, d = c.rsplit(":", 3)
        cases.append((factory, int(S), int(rows), int(d)))
    for factory, S, rows, d in cases:
        x, q = corpus("clustered", S * rows, d, 64, 1.0, S * rows + d)
        q = np.ascontiguousarray(q[:a.nq])
        nq = len(q)
        with tempfile.TemporaryDirectory(dir=a.dir) as root:
            used = build_shards(pkg, root, now, factory, S, rows, d, m, x, a.niter, a.niter_opq)
            sh = ff.HourlyShardedIndex(m, d, root, S, S)
            sh.reload(now)
            assert len(sh.directories) == S
            for k in [int(v) for v in a.ks.split(",")]:
                for _ in range(a.warmup):
                    want = sh.search_composed(q, k, a.nprobe)
                    got = sh.search(q, k, a.nprobe)
                same = all(u.tobytes() == v.tobytes() for u, v in zip(got, want))
                t_set, t_comp = [], []
                for _ in range(a.reps):  # alternating, each call ends with its answer on the host
                    t0 = time.perf_counter()
                    sh.search_composed(q, k, a.nprobe)
                    t_comp.append(1e3 * (time.perf_counter() - t0))
                    t0 = time.perf_counter()
                    sh.search(q, k, a.nprobe)
                    t_set.append(1e3 * (time.perf_counter() - t0))
                st = sh.last_stats()
                line = {"factory": used, "shards": S, "rows_per_shard": rows, "dim": d, "metric": a.metric, "nq": nq, "k": k,
                        "nprobe": a.nprobe, "warmup": a.warmup, "reps": a.reps,
                        "set_ms": round(statistics.median(t_set), 3), "set_ms_min": round(min(t_set), 3), "set_ms_max": round(max(t_set), 3),
                        "composed_ms": round(statistics.median(t_comp), 3), "composed_ms_min": round(min(t_comp), 3),
                        "composed_ms_max": round(max(t_comp), 3),
                        "search_ms": round(st["search_ms"], 3), "fold_ms": round(st["fold_ms"], 3),
                        "set_h2d_bytes": st["h2d_bytes"], "set_d2h_bytes": st["d2h_bytes"], "set_d2h_result_bytes": st["d2h_result_bytes"],
                        "composed_h2d_bytes": S * 4 * nq * d, "composed_d2h_result_bytes": S * (12 * nq * k + 4 * nq),
                        "same_answers": same}
                print(json.dumps(line), flush=True)
            sh.close()


if __name__ == "__main__":
    main()
