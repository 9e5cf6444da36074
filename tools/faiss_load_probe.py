"""What loading a saved index costs (include/faiss_files.h) against building it again, at the same commit in the same process.
For each of IVF<nlist>,Flat / IVF<nlist>,PQ<M> / OPQ<M>,IVF<nlist>,PQ<M> over n rows of dimension dim, one entry of the one
JSON line:
  build_s      train on the first n_train rows + add of all rows (what a service without the file would have to repeat),
               the better of two builds; before the first kind a small throwaway index is built, saved and loaded, so that
               neither side pays for the HIP context and the code objects
  save_s       write_index to a fresh directory
  file_bytes, bytes_per_row   the size of faiss.index, and that size over n
  load_s       FaissIndex.load_index of the directory: the best of --reps loads (the file is in the page cache after the
               first; load_first_s is the first) -- each load ends with the lists laid out and the device synchronised
  same_answers the loaded index answers nq queries byte for byte as the built one
  speedup_first, speedup   build_s / load_first_s (the file read from storage, if it was not cached) and build_s / load_s

Run it under its own time limit, e.g.
  timeout -k 10 1200 python tools/faiss_load_probe.py --n 1000000 --dim 256 > profiles/faiss_load_probe_1M_d256.json"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ivf_probe import corpus  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", default="clustered", choices=["clustered", "iid"])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--M", type=int, default=32)
    ap.add_argument("--n-train", type=int, default=0)
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--niter-opq", type=int, default=10)
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--metric", default="Cosine")
    ap.add_argument("--kinds", default="flat,pq,opq")
    ap.add_argument("--dir", default=None, help="where the directories are written (default: a temporary directory)")
    a = ap.parse_args()
    pkg = load_package()
    ff = pkg.faiss_files
    m = getattr(pkg.dense_ann.DistanceMetric, a.metric)
    n, d = a.n, a.dim
    x, q = corpus(a.corpus, n, d, max(1, a.nlist // 4), 1.0, n + len(a.corpus))
    q = q[:a.nq]
    n_train = min(n, a.n_train or 64 * a.nlist)
    line = {"corpus": a.corpus, "metric": a.metric, "n": n, "dim": d, "nlist": a.nlist, "M": a.M, "n_train": n_train,
            "niter": a.niter, "niter_opq": a.niter_opq, "nq": len(q), "k": a.k, "nprobe": a.nprobe, "reps": a.reps}

    def build(kind):
        if kind == "flat":
            ix = pkg.ivf_ann.FaissIvfFlat.train(m, a.nlist, x[:n_train], niter=a.niter, seed=1)
        elif kind == "pq":
            ix = pkg.ivfpq_ann.FaissIvfPq.train(m, a.nlist, a.M, x[:n_train], niter=a.niter, seed=1)
        else:
            ix = pkg.opq_ann.FaissOpqIvfPq.train(m, a.nlist, a.M, d, x[:n_train], niter=a.niter, niter_opq=a.niter_opq, seed=1)
        ix.add(x)
        return ix

    with tempfile.TemporaryDirectory(dir=a.dir) as root:
        # warm the device: context, code objects and allocator, through every path timed below
        for kind in a.kinds.split(","):
            if kind == "flat":
                w = pkg.ivf_ann.FaissIvfFlat.train(m, 8, x[:4096], niter=1, seed=1)
            elif kind == "pq":
                w = pkg.ivfpq_ann.FaissIvfPq.train(m, 8, a.M, x[:4096], niter=1, seed=1)
            else:
                w = pkg.opq_ann.FaissOpqIvfPq.train(m, 8, a.M, d, x[:4096], niter=1, niter_opq=1, seed=1)
            w.add(x[:4096])
            ff.write_index(w, os.path.join(root, "warm_" + kind))
            w.close()
            ff.FaissIndex.load_index(d, m, os.path.join(root, "warm_" + kind)).index.close()
        for kind in a.kinds.split(","):
            builds = []
            for rep in range(2):
                t0 = time.perf_counter()
                ix = build(kind)
                builds.append(time.perf_counter() - t0)
                if rep == 0:
                    ix.close()
            build_s = min(builds)
            want = ix.search(q, a.k, a.nprobe)
            directory = os.path.join(root, kind)
            t0 = time.perf_counter()
            ff.write_index(ix, directory)
            save_s = time.perf_counter() - t0
            ix.close()
            size = os.path.getsize(os.path.join(directory, ff.INDEX_FILE_NAME))
            loads, same = [], True
            for _ in range(a.reps):
                t0 = time.perf_counter()
                back = ff.FaissIndex.load_index(d, m, directory).index
                loads.append(time.perf_counter() - t0)
                got = back.search(q, a.k, a.nprobe)
                same = same and all(u.tobytes() == v.tobytes() for u, v in zip(want, got))
                back.close()
            line[kind] = {"build_s": round(build_s, 3), "save_s": round(save_s, 3), "file_bytes": size,
                          "bytes_per_row": round(size / n, 2), "load_first_s": round(loads[0], 3), "load_s": round(min(loads), 3),
                          "same_answers": same, "speedup_first": round(build_s / loads[0], 1),
                          "speedup": round(build_s / min(loads), 1)}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
