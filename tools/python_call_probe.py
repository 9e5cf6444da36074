"""What one call through the Python binding costs on the host, without a device: search() of the five index classes on an
object made with a null handle.  The library refuses a null handle before any HIP call, so a call is the whole wrapper path
-- the row check, the result arrays, the ctypes call, the status turned into the module's error -- and nothing else.

One JSON line per class and repeat: {"call", "repeat", "calls", "us_per_call"}.  3 queries of d = 16, k = 10.

Run it at two commits in turns (the same built library for both, through SANN_LIB_PATH), e.g.
  python tools/python_call_probe.py --repeats 1 --repeat-index 0 >> profiles/python_binding_cpu_calls_change.jsonl"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--repeat-index", type=int, default=0, help="the number of the first repeat, for runs taken in turns")
    a = ap.parse_args()
    pkg = load_package()
    L2 = pkg.dense_ann.DistanceMetric.L2
    q = np.random.default_rng(1).standard_normal((3, 16)).astype(np.float32)
    cases = [
        ("FaissIvfFlat.search", pkg.ivf_ann.FaissIvfFlat(None, L2, 16, 4), (q, 10, 4), pkg.ivf_ann.IvfError),
        ("FaissIvfPq.search", pkg.ivfpq_ann.FaissIvfPq(None, L2, 16, 4, 4), (q, 10, 4), pkg.ivfpq_ann.IvfPqError),
        ("FaissOpqIvfPq.search", pkg.opq_ann.FaissOpqIvfPq(None, L2, 16, 16, 4, 4), (q, 10, 4), pkg.opq_ann.OpqError),
        ("Hnsw.search", pkg.hnsw_ann.Hnsw(None, L2, 10, 16, 8), (q, 10, 50), pkg.hnsw_ann.HnswError),
        ("BruteForceIndex.search", pkg.dense_ann.BruteForceIndex(None, L2, 10, 16), (q, 10), pkg.dense_ann.DannError),
    ]
    for name, index, args, error in cases:  # the first call loads the library and attaches the module's prototypes
        try:
            index.search(*args)
        except error:
            pass
    for r in range(a.repeats):
        for name, index, args, error in cases:
            search = index.search
            t0 = time.perf_counter()
            for _ in range(a.calls):
                try:
                    search(*args)
                except error:
                    continue
                raise SystemExit(f"{name}: a null handle was not refused")
            dt = time.perf_counter() - t0
            print(json.dumps({"call": name, "repeat": a.repeat_index + r, "calls": a.calls, "us_per_call": round(1e6 * dt / a.calls, 4)}),
                  flush=True)


if __name__ == "__main__":
    main()
