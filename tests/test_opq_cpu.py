"""The OPQ pre-transform (include/opq_ann.h) without a GPU: the exported symbols, index_factory, the default factory string,
the host's Procrustes step against numpy's SVD, and the index build with the training call replaced."""
import os
import re

import numpy as np
import pytest

import _opq_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(pkg):
    lib = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "opq_ann.h")).read()
    declared = set(re.findall(r"\b(opq_[a-z_0-9]+)\s*\(", header.split("#ifndef OPQ_ANN_H")[1]))
    assert len(declared) >= 20, "declarations parsed"
    assert declared == set(pkg.opq_ann.PROTOS)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/opq_ann.h but not exported"
    # the device-rows seam into the two inverted-file indexes is internal: none of it is a dynamic symbol
    import subprocess
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "the-algorithm_amd", "libsimclusters_amd.so")],
                          capture_output=True, text=True, check=True).stdout
    assert "ivfpq_internal" not in syms and "ivf_internal" not in syms


def test_index_factory_strings(pkg):
    oq, pq = pkg.opq_ann, pkg.ivfpq_ann
    m = pkg.dense_ann.DistanceMetric
    spec = oq.index_factory(256, "OPQ48_240,IVF1024,PQ48", m.Cosine)
    assert (spec.dimension, spec.d_out, spec.nlist, spec.M, spec.metric) == (256, 240, 1024, 48, m.Cosine)
    assert spec.index_class is oq.FaissOpqIvfPq
    spec = oq.index_factory(64, "OPQ16,IVF64,PQ16", m.L2)
    assert (spec.dimension, spec.d_out, spec.nlist, spec.M) == (64, 64, 64, 16)
    spec = oq.index_factory(64, "OPQ16_32,IVF8,PQ16x8", m.InnerProduct)
    assert (spec.d_out, spec.M) == (32, 16)
    for d, bad in [(64, "OPQ8,IVF64,PQ16"),        # the two M differ
                   (64, "OPQ16_128,IVF64,PQ16"),   # dout > dimension
                   (64, "OPQ16_40,IVF64,PQ16"),    # dout % M != 0
                   (64, "OPQ8_24,IVF64,PQ8"),      # the inner shape: 24 is no multiple of 16
                   (64, "OPQ2_32,IVF64,PQ2"),      # the inner shape: M = 2
                   (64, "OPQ16,IVF0,PQ16"),        # the inner shape: nlist = 0
                   (2048, "OPQ16_64,IVF8,PQ16")]:  # the input dimension
        with pytest.raises(ValueError) as e:
            oq.index_factory(d, bad, m.L2)
        assert repr(bad) in str(e.value), "the message names the string"
    # every other string is ivfpq_ann.index_factory's
    for s in ["IVF1024,Flat", "IVF4096,PQ32", "IVF16,PQ64x8"]:
        a, b = oq.index_factory(256, s, m.Cosine), pq.index_factory(256, s, m.Cosine)
        assert type(a) is type(b) and vars(a) == vars(b)
    for bad in ["", "OPQ16,IVF64,Flat", "OPQ16,IVF64", "opq16,IVF64,PQ16", "OPQ16,IVF64,PQ16x4", "OPQ16_,IVF64,PQ16", None]:
        with pytest.raises(ValueError) as e:
            oq.index_factory(64, bad, m.L2)
        assert repr(bad) in str(e.value)
    with pytest.raises(ValueError):
        pq.index_factory(64, "OPQ16,IVF64,PQ16", m.L2)  # the IVF-PQ factory still serves no OPQ string


def test_default_factory_string(pkg):
    oq = pkg.opq_ann
    assert oq.default_factory_string(2000, 256) == "OPQ48_240,IVF100,PQ48"
    assert oq.default_factory_string(2000, 96) == "OPQ48,IVF100,PQ48"
    for n, d in [(2000, 256), (2000, 96), (1_000_000, 200), (39, 48), (41, 144)]:
        assert oq.default_factory_string(n, d) == ref.default_factory_string(n, d)
    spec = oq.index_factory(256, oq.default_factory_string(20480, 256), pkg.dense_ann.DistanceMetric.Cosine)
    assert (spec.d_out, spec.nlist, spec.M) == (240, 1024, 48), "the device serves the reference's default shape at d = 256"


def _rank_deficient(rng, d_in, d_out, rank):
    return rng.standard_normal((d_in, rank)) @ rng.standard_normal((rank, d_out))


@pytest.mark.parametrize("case", ["16x16", "40x32", "256x240", "rank-deficient", "zero"])
def test_procrustes_against_numpy_svd(pkg, case):
    rng = np.random.default_rng(5)
    if case == "rank-deficient":
        C = _rank_deficient(rng, 40, 32, 7)
    elif case == "zero":
        C = np.zeros((40, 32))
    else:
        d_in, d_out = (int(s) for s in case.split("x"))
        C = rng.standard_normal((d_in, d_out))
    A = pkg.opq_ann.procrustes(C)
    assert A.shape == (C.shape[1], C.shape[0]) and np.all(np.isfinite(A))
    gram_err = np.abs(A @ A.T - np.eye(C.shape[1])).max()
    _, nuclear = ref.procrustes(C)
    trace = float(np.trace(A @ C))
    print(f"{case}: |A A^T - I| = {gram_err:.3e}, tr(A C) / sum sigma = {trace / nuclear if nuclear else 1.0:.15f}")
    assert gram_err <= 1e-12
    assert trace >= (1 - 1e-10) * nuclear, "the Procrustes maximum is the nuclear norm"
    assert pkg.opq_ann.procrustes(C).tobytes() == A.tobytes(), "two calls are byte-identical"


def test_procrustes_refuses_bad_arguments(pkg):
    oq = pkg.opq_ann
    with pytest.raises(ValueError):
        oq.procrustes(np.zeros((16, 32)))  # d_out > d_in
    with pytest.raises(oq.OpqError, match="finite"):
        oq.procrustes(np.full((16, 16), np.nan))
    lib = oq._lib()
    assert lib.opq_procrustes(16, 16, None, None) == 1 and b"null" in lib.opq_last_error()


def test_build_faiss_index_with_the_training_replaced(pkg, monkeypatch):
    oq = pkg.opq_ann
    m = pkg.dense_ann.DistanceMetric
    calls = []

    class _Index:
        def add(self, v, ids):
            calls.append(("add", v.shape, list(ids)))

    def fake_train(cls, metric, nlist, M, d_out, v, *, niter, niter_opq, seed, device):
        calls.append(("train", cls.__name__, metric, nlist, M, d_out, v.shape, niter, niter_opq, seed))
        return _Index()

    def fake_pq_train(cls, metric, nlist, M, v, *, niter, seed, device):
        calls.append(("train", cls.__name__, metric, nlist, M, v.shape, niter, seed))
        return _Index()

    monkeypatch.setattr(oq.FaissOpqIvfPq, "train", classmethod(fake_train))
    monkeypatch.setattr(pkg.ivfpq_ann.FaissIvfPq, "train", classmethod(fake_pq_train))
    x = np.arange(40 * 48, dtype=np.float32).reshape(40, 48)
    out = oq.build_faiss_index(x, range(40), 0.25, "OPQ8_32,IVF2,PQ8", m.L2, niter_opq=3)
    assert isinstance(out, _Index)
    assert calls[0] == ("train", "FaissOpqIvfPq", m.L2, 2, 8, 32, (10, 48), 0, 3, 1), "the first trainingSetSize rows"
    assert calls[1] == ("add", (40, 48), list(range(40))), "all rows are added"
    # no string: the reference's default, here OPQ48,IVF2,PQ48 (48 divides the dimension; 40 rows / 20)
    del calls[:]
    oq.build_faiss_index(x, range(40), 0.5, None, m.Cosine)
    assert calls[0] == ("train", "FaissOpqIvfPq", m.Cosine, 2, 48, 48, (20, 48), 0, 0, 1)
    # a string without OPQ builds what ivfpq_ann builds
    del calls[:]
    oq.build_faiss_index(x, range(40), 0.25, "IVF2,PQ4", m.L2)
    assert calls[0] == ("train", "FaissIvfPq", m.L2, 2, 4, (10, 48), 0, 1)
    with pytest.raises(ValueError, match="OPQ8_32,IVF2,PQ4"):
        oq.build_faiss_index(x, range(40), 0.25, "OPQ8_32,IVF2,PQ4", m.L2)
