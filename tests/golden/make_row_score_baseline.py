"""Generator of tests/golden/row_score_baseline.npz: the bytes the re-rank (refine_ann.hip) and the Annoy index
(annoy_ann.hip) answered at the commit before both took the distance of a (query, stored fp16 row) pair from
csrc/row_score.h.  Beyond the refine_* block of ivf_family_baseline.npz (d = 64: one piece, fewer than 64 lanes busy) it
covers the row widths at which the kernels take another path -- d = 3 (one partial piece; Annoy only, below the OPQ base's
16), 100 (padding to 104), 200 (25 pieces), 1024 (two pieces a lane) -- on N = 1500 rows added in two calls with caller ids
and 8 queries:

  refine_<d>_<metric>_<k>_<k_factor>_*   FaissRefineFlat.wrap(FaissOpqIvfPq.load(metric, A, cent, cb), k_factor=4), A an
            integer matrix / 16 as in make_pq_search_baseline.inputs("opq"), D_OUT = 64, M = 8, NLIST = 16; every SEARCHES
            entry at nprobe 16: ids, dist, cnt.  (256, 4) hands the re-rank 1024 candidates, the full sort.
  annoy_<d>_<metric>_<k>_<nodes_to_explore>_*   AnnoyQueryable.from_forest(AnnoyForest.build(metric, x, 7, 0, seed=3), x,
            ids): ids, dist, cnt, and pops and collected of last_stats().  The one (100, L2, 1024, 20000) search hands the
            selection more than 1024 candidates (its radix passes).
  annoy_<d>_<metric>_{forest,rows}_sha256   digests of the forest's arrays and of rows(): host code, so a host-side
            difference is told apart from a kernel difference.

Every input is a small dyadic rational made from integer draws (make_pq_search_baseline._rows), every transform an explicit
sum in a fixed order: nothing depends on a linear-algebra library.  tests/test_refine_gpu.py and tests/test_annoy_gpu.py each
recompute their blocks and ask for byte-equal arrays.  The generator refuses to write unless every (256, 4) search filled
1024 candidates, the k = 1024 Annoy search had more than 1024 candidates for both queries and every block holds a non-zero
distance.

usage (on a card, at the baseline commit): python tests/golden/make_row_score_baseline.py [dest_dir]
"""
import hashlib
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_pq_search_baseline", os.path.join(HERE, "make_pq_search_baseline.py"))
_base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_base)
_rows = _base._rows

N, NQ, NLIST, M, D_OUT = 1500, 8, 16, 8, 64
FIRST_ADD = 900
REFINE_DIMS = [100, 200, 1024]
REFINE_METRICS = ["L2", "Cosine", "InnerProduct"]
REFINE_NPROBE, REFINE_K_FACTOR = 16, 4
SEARCHES = [(1, 1, NQ), (10, 8, NQ), (256, 4, 2)]  # (k, k_factor, the first so many queries)
ANNOY_DIMS = [3, 100, 200, 1024]
ANNOY_METRICS = ["L2", "Cosine"]
ANNOY_TREES, ANNOY_SEED, ANNOY_K = 7, 3, 10
ANNOY_WIDE = (100, "L2", 1024, 20000, 2)  # (d, metric, k, nodes_to_explore, the first so many queries)


def _metric(pkg, name):
    return getattr(pkg.dense_ann.DistanceMetric, name)


def data(d):
    """(x [N, d], caller ids, queries [NQ, d]) of a row width."""
    rng = np.random.default_rng(20250 + d)
    x = _rows(rng, N + NQ, d)
    return x[:N], rng.permutation(N).astype(np.int64) * 3 + 5, x[N:]


def opq_base(d):
    """(A [D_OUT, d], centroids [NLIST, D_OUT], codebooks) as make_pq_search_baseline.inputs("opq") makes them."""
    rng = np.random.default_rng(20260 + d)
    x = data(d)[0]
    cb = (rng.integers(-32, 33, (M, 256, D_OUT // M)).astype(np.float64) / 64.0).astype(np.float32)
    A = (rng.integers(-4, 5, (D_OUT, d)).astype(np.float64) / 16.0).astype(np.float32)
    y = np.zeros((NLIST, D_OUT))
    for i in range(d):  # (an explicit sum in a fixed order: no BLAS)
        y += x[:NLIST, i:i + 1].astype(np.float64) * A[:, i].astype(np.float64)[None, :]
    return A, y.astype(np.float32), cb


def refine_answers(pkg):
    """(arrays of the refine_* blocks, {search name: the candidate counts the re-rank was handed})."""
    out, handed = {}, {}
    for d in REFINE_DIMS:
        x, ids, q = data(d)
        for metric in REFINE_METRICS:
            base = pkg.opq_ann.FaissOpqIvfPq.load(_metric(pkg, metric), *opq_base(d))
            ix = pkg.refine_ann.FaissRefineFlat.wrap(base, k_factor=REFINE_K_FACTOR)
            ix.add(x[:FIRST_ADD], ids[:FIRST_ADD])
            ix.add(x[FIRST_ADD:], ids[FIRST_ADD:])
            for k, kf, nq in SEARCHES:
                name = f"refine_{d}_{metric}_{k}_{kf}"
                out[name + "_ids"], out[name + "_dist"], out[name + "_cnt"] = ix.search(q[:nq], k, REFINE_NPROBE, kf)
                handed[name] = ix.last_candidates()[1]
            ix.close()
    return out, handed


def _sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def annoy_answers(pkg):
    """(arrays of the annoy_* blocks, {search name: the candidate counts the selection was handed})."""
    an = pkg.annoy_ann
    out, handed = {}, {}
    for d in ANNOY_DIMS:
        x, ids, q = data(d)
        for metric in ANNOY_METRICS:
            f = an.AnnoyForest.build(_metric(pkg, metric), x, ANNOY_TREES, 0, seed=ANNOY_SEED)
            ix = an.AnnoyQueryable.from_forest(f, x, ids)
            out[f"annoy_{d}_{metric}_forest_sha256"] = _sha256(f.nodes, f.normals, f.offsets, f.roots, f.items)
            out[f"annoy_{d}_{metric}_rows_sha256"] = _sha256(ix.rows())
            searches = [(ANNOY_K, None, NQ)] + ([ANNOY_WIDE[2:]] if (d, metric) == ANNOY_WIDE[:2] else [])
            for k, nte, nq in searches:
                name = f"annoy_{d}_{metric}_{k}_{nte}"
                out[name + "_ids"], out[name + "_dist"], out[name + "_cnt"] = ix.search(q[:nq], k, nte)
                st = ix.last_stats()
                out[name + "_pops"], out[name + "_collected"] = st["pops"], st["collected"]
                handed[name] = ix.last_candidates()[1]
            ix.close()
            f.close()
    return out, handed


def check(out, handed):
    """The conditions without which nothing is written."""
    for name, cnt in handed.items():
        if name.startswith("refine_") and name.endswith("_256_4"):
            assert np.all(cnt == 1024), f"{name}: the re-rank was handed {cnt.tolist()} candidates, not 1024"
    wide = "annoy_%d_%s_%d_%d" % ANNOY_WIDE[:4]
    assert len(handed[wide]) == 2 and np.all(handed[wide] > 1024), f"{wide}: {handed[wide].tolist()} candidates"
    blocks = {}  # "<kind>_<d>_<metric>" -> some distance of the block is not zero
    for name in out:
        if name.endswith("_dist"):
            block = "_".join(name.split("_")[:3])
            blocks[block] = blocks.get(block, False) or bool(out[name].any())
    assert len(blocks) == len(REFINE_DIMS) * len(REFINE_METRICS) + len(ANNOY_DIMS) * len(ANNOY_METRICS)
    assert all(blocks.values()), f"every distance is zero in {[b for b, some in blocks.items() if not some]}"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    from _pkg import load_package

    package = load_package()
    dest = sys.argv[1] if len(sys.argv) > 1 else HERE
    r_out, r_handed = refine_answers(package)
    a_out, a_handed = annoy_answers(package)
    everything, counts = {**r_out, **a_out}, {**r_handed, **a_handed}
    for name_ in sorted(counts):
        print(name_, "candidates", counts[name_].tolist(), "answered", everything[name_ + "_cnt"].tolist())
    check(everything, counts)
    path = os.path.join(dest, "row_score_baseline.npz")
    np.savez_compressed(path, **everything)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 128 * 1024, "the fixture must stay under 128 KB"
