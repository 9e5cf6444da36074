"""Generator of tests/golden/ivfpq_search_baseline.npz and tests/golden/opq_search_baseline.npz: the answers of ivfpq_search
and opq_search on small indexes loaded from numpy-made centroids, codebooks and matrices, as the library gave them at the
commit before the select step gained its position-writing variant (refine_ann.h's seam, ivfpq_internal::search_positions).
tests/test_refine_gpu.py builds the same indexes from inputs() and asks for byte-equal answers.

Every input is a small dyadic rational made from integer draws, so the arrays are bit-identical on every machine and numpy
version; nothing here depends on a linear-algebra library's order of summation.

usage (on a card, at the baseline commit): python tests/golden/make_pq_search_baseline.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
METRICS = ["L2", "Cosine", "InnerProduct"]
SEARCHES = [(10, 4), (64, 16)]  # (k, nprobe)
N, NQ, NLIST, M = 2000, 8, 16, 8
D, D_IN, D_OUT = 64, 72, 64


def _rows(rng, n, d):
    """Latent rows of dimension 3 under an integer map into R^d plus small noise: all exact in float32."""
    latent = rng.integers(-64, 65, (n, 3)).astype(np.float64) / 32.0
    basis = rng.integers(-32, 33, (3, d)).astype(np.float64) / 32.0
    noise = rng.integers(-16, 17, (n, d)).astype(np.float64) / 64.0
    out = np.zeros((n, d))
    for r in range(3):  # (an explicit sum in a fixed order: no BLAS)
        out += latent[:, r:r + 1] * basis[r][None, :]
    return (out + noise).astype(np.float32)


def inputs(kind):
    """kind 'ivfpq': (x [N, D], ids, queries, centroids, codebooks); kind 'opq': the same at D_IN with the matrix last."""
    rng = np.random.default_rng(20240 if kind == "ivfpq" else 20241)
    d = D if kind == "ivfpq" else D_IN
    x = _rows(rng, N + NQ, d)
    x, q = x[:N], x[N:]
    ids = rng.permutation(N).astype(np.int64) * 3 + 5
    cb = (rng.integers(-32, 33, (M, 256, D_OUT // M)).astype(np.float64) / 64.0).astype(np.float32)
    if kind == "ivfpq":
        return x, ids, q, x[:NLIST].copy(), cb
    A = (rng.integers(-4, 5, (D_OUT, D_IN)).astype(np.float64) / 16.0).astype(np.float32)
    y = np.zeros((NLIST, D_OUT))
    for i in range(D_IN):
        y += x[:NLIST, i:i + 1].astype(np.float64) * A[:, i].astype(np.float64)[None, :]
    return x, ids, q, y.astype(np.float32), cb, A


def build(pkg, kind, metric):
    m = getattr(pkg.dense_ann.DistanceMetric, metric)
    if kind == "ivfpq":
        x, ids, q, cent, cb = inputs(kind)
        ix = pkg.ivfpq_ann.FaissIvfPq.load(m, cent, cb)
    else:
        x, ids, q, cent, cb, A = inputs(kind)
        ix = pkg.opq_ann.FaissOpqIvfPq.load(m, A, cent, cb)
    ix.add(x[:1200], ids[:1200])
    ix.add(x[1200:], ids[1200:])
    return ix, q


def answers(pkg, kind):
    """{'<metric>_<k>_<nprobe>_{ids,dist,cnt}': array} of every search of the baseline."""
    out = {}
    for metric in METRICS:
        ix, q = build(pkg, kind, metric)
        for k, nprobe in SEARCHES:
            ids, dist, cnt = ix.search(q, k, nprobe)
            out[f"{metric}_{k}_{nprobe}_ids"] = ids
            out[f"{metric}_{k}_{nprobe}_dist"] = dist
            out[f"{metric}_{k}_{nprobe}_cnt"] = cnt
        ix.close()
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    from _pkg import load_package

    package = load_package()
    dest = sys.argv[1] if len(sys.argv) > 1 else HERE
    for kind_ in ("ivfpq", "opq"):
        path = os.path.join(dest, f"{kind_}_search_baseline.npz")
        np.savez_compressed(path, **answers(package, kind_))
        print("wrote", path, os.path.getsize(path), "bytes")
