"""What the one-shot device build leaves on the device: free device memory before the 1M x 256 build and after it returns
(before any search), the build's time, and the times of the first graph export, which reads the lists back from the device,
and of a second one straight after it, which does not have to.
One JSON line; `label` names the tree when two are compared."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402


def main():
    label = sys.argv[1] if len(sys.argv) > 1 else ""
    pkg = load_package()
    pkg.load_library()
    import torch

    m = pkg.dense_ann.DistanceMetric.Cosine
    x = np.random.default_rng(0).standard_normal((1_000_000, 256), dtype=np.float32)
    torch.cuda.init()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    t0 = time.perf_counter()
    ix = pkg.hnsw_ann.Hnsw.build(m, x, max_m=16, ef_construction=200, seed=1, gpu=True)
    build_s = time.perf_counter() - t0
    free1, _ = torch.cuda.mem_get_info()
    t0 = time.perf_counter()
    g = ix.graph()
    graph_s = time.perf_counter() - t0
    free2, _ = torch.cuda.mem_get_info()
    t0 = time.perf_counter()
    ix.graph()
    repeat_s = time.perf_counter() - t0
    ids, _, _ = ix.search(x[:256], 10, 100)
    print(json.dumps({"what": "build_memory", "tree": label, "free_before": free0, "free_after_build": free1, "used_by_build": free0 - free1,
                      "free_after_first_export": free2, "build_s": build_s, "first_graph_s": graph_s,
                      "repeat_graph_s": repeat_s, "build_plus_first_export_s": build_s + graph_s, "graph_entries": int(len(g[0])), "graph_neighbours": int(len(g[3])),
                      "self_hits_of_256": int((ids[:, 0] == np.arange(256)).sum()), "build_stats": list(ix.build_stats())}), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
