"""The re-ranking index (include/refine_ann.h) without a GPU: the exported symbols, argument errors that return before any
device call, the factory strings, the CPU restatement tests/_refine_ref.py against answers derived by hand, and the input of
the quality test of tests/test_refine_gpu.py, fixed here by numpy alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _refine_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1

from _refine_ref import QUALITY, QUALITY_SEED


def test_library_exports_every_declared_symbol(pkg):
    lib = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "refine_ann.h")).read()
    declared = set(re.findall(r"\b(refine_[a-z_0-9]+)\s*\(", header))
    assert len(declared) >= 13, "declarations parsed"
    assert declared == set(pkg.refine_ann.PROTOS)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/refine_ann.h but not exported"


def test_argument_errors_return_before_any_device_call(pkg):
    lib = pkg.refine_ann._lib()
    h = C.c_void_p()
    x = np.zeros((4, 64), np.float32)
    out = np.zeros(2048, np.int64)
    fake = C.create_string_buffer(4096)  # the numbers are refused before the handle is looked at
    addr = C.addressof(fake)

    def err():
        return lib.refine_last_error().decode()

    def search(handle=addr, nq=1, q=x.ctypes.data, k=1, nprobe=1, kf=1, dist=out.ctypes.data, ids=out.ctypes.data, cnt=out.ctypes.data):
        return lib.refine_search_with_k_factor(handle, nq, q, k, nprobe, kf, dist, ids, cnt)

    assert search(k=205, kf=5) == EINVAL and "1025" in err() and "k_factor" in err(), "k * k_factor = 1025"
    assert search(k=1025, kf=1) == EINVAL and "k must" in err()
    assert search(k=1, kf=1025) == EINVAL and "k_factor" in err()
    assert search(k=1, kf=0) == EINVAL and "k_factor" in err()
    assert search(k=0) == EINVAL and search(nq=0) == EINVAL
    assert search(nprobe=0) == EINVAL and "nprobe" in err()
    assert search(nprobe=1025) == EINVAL
    assert search(handle=None) == EINVAL and "null" in err()
    assert search(q=None) == EINVAL and search(dist=None) == EINVAL and search(ids=None) == EINVAL and search(cnt=None) == EINVAL
    assert lib.refine_search(None, 1, x.ctypes.data, 1, 1, out.ctypes.data, out.ctypes.data, out.ctypes.data) == EINVAL
    # wrapping: k_factor 0 and 1025, NULL base, NULL out
    for wrap in (lib.refine_index_wrap_ivfpq, lib.refine_index_wrap_opq):
        assert wrap(addr, 0, C.byref(h)) == EINVAL and "k_factor" in err()
        assert wrap(addr, 1025, C.byref(h)) == EINVAL and "k_factor" in err()
        assert wrap(None, 1, C.byref(h)) == EINVAL and "null" in err()
        assert wrap(addr, 1, None) == EINVAL and "null" in err()
    assert h.value is None
    assert lib.refine_index_set_k_factor(addr, 0) == EINVAL and lib.refine_index_set_k_factor(addr, 1025) == EINVAL
    assert lib.refine_index_set_k_factor(None, 4) == EINVAL and "null" in err()
    assert lib.refine_index_add(None, 1, x.ctypes.data, None) == EINVAL and "null" in err()
    assert lib.refine_index_info(None, None, None, None, None, None) == EINVAL
    assert lib.refine_index_base(None, None, None) == EINVAL
    assert lib.refine_last_candidates(None, None, None, None, None) == EINVAL
    assert lib.refine_index_get_rows(None, 0, 0, None) == EINVAL
    assert lib.refine_last_stats(None, None, None) == EINVAL
    assert lib.refine_index_destroy(None) == 0
    with pytest.raises(TypeError, match="FaissIvfPq"):
        pkg.refine_ann.FaissRefineFlat.wrap(object())


def test_index_factory_strings(pkg):
    rf, opq, pq = pkg.refine_ann, pkg.opq_ann, pkg.ivfpq_ann
    m = pkg.dense_ann.DistanceMetric
    spec = rf.index_factory(64, "IVF64,PQ8,RFlat", m.L2, k_factor=4)
    assert isinstance(spec, rf.RefineIndexSpec) and spec.index_class is rf.FaissRefineFlat and spec.k_factor == 4
    assert isinstance(spec.base_spec, pq.IndexSpec) and (spec.base_spec.nlist, spec.base_spec.M) == (64, 8)
    assert (spec.dimension, spec.metric, spec.factory_string) == (64, m.L2, "IVF64,PQ8,RFlat")
    spec = rf.index_factory(72, "OPQ8_64,IVF64,PQ8,Refine(Flat)", m.Cosine)
    assert isinstance(spec, rf.RefineIndexSpec) and spec.k_factor == 1 and isinstance(spec.base_spec, opq.OpqIndexSpec)
    assert (spec.base_spec.d_out, spec.base_spec.nlist, spec.base_spec.M, spec.dimension) == (64, 64, 8, 72)
    assert isinstance(rf.index_factory(64, "IVF64,PQ8x8,RFlat", m.L2).base_spec, pq.IndexSpec)
    for bad in ["IVF64,Flat,RFlat", "IVF64,PQ8,RFlat ", "IVF64,PQ8,Rflat", "IVF64,PQ8,Refine(PQ8)", "IVF64,PQ8,RFlat,RFlat", ",RFlat",
                "RFlat", "OPQ8_64,IVF64,PQ16,RFlat", None]:
        with pytest.raises(ValueError) as e:
            rf.index_factory(64, bad, m.L2)
        assert repr(bad) in str(e.value), "the message names the string"
    for kf in (0, 1025):
        with pytest.raises(ValueError, match="k_factor"):
            rf.index_factory(64, "IVF64,PQ8,RFlat", m.L2, k_factor=kf)
    # every other string is opq_ann.index_factory's, unchanged
    plain = rf.index_factory(64, "IVF64,PQ8", m.L2)
    assert isinstance(plain, pq.IndexSpec) and plain.index_class is pq.FaissIvfPq
    assert rf.index_factory(64, "IVF64,Flat", m.L2).index_class is pkg.ivf_ann.FaissIvfFlat
    assert isinstance(rf.index_factory(64, "OPQ8,IVF64,PQ8", m.L2), opq.OpqIndexSpec)
    with pytest.raises(ValueError, match="k_factor"):
        rf.index_factory(64, "IVF64,PQ8", m.L2, k_factor=2)
    # the older factories keep refusing the suffix
    for factory in (pq.index_factory, opq.index_factory):
        for s in ("IVF64,PQ8,RFlat", "IVF64,PQ8,Refine(Flat)", "OPQ8,IVF64,PQ8,RFlat"):
            with pytest.raises(ValueError):
                factory(64, s, m.L2)


def test_build_restates_the_indexer(pkg, monkeypatch):
    rf, opq, pq = pkg.refine_ann, pkg.opq_ann, pkg.ivfpq_ann
    m = pkg.dense_ann.DistanceMetric
    calls = []

    class _Base:
        def close(self):
            calls.append(("close",))

        def add(self, v, ids):
            calls.append(("base add", v.shape, list(ids)))

    class _Index:
        def add(self, v, ids):
            calls.append(("add", v.shape, list(ids)))

    def fake_pq_train(cls, metric, nlist, M, v, *, niter, seed, device):
        calls.append(("train", "FaissIvfPq", metric, nlist, M, v.shape, niter, seed))
        return _Base()

    def fake_opq_train(cls, metric, nlist, M, d_out, v, *, niter, niter_opq, seed, device):
        calls.append(("train", "FaissOpqIvfPq", metric, nlist, M, d_out, v.shape, niter, niter_opq, seed))
        return _Base()

    def fake_wrap(cls, base, k_factor=1):
        calls.append(("wrap", type(base).__name__, k_factor))
        return _Index()

    monkeypatch.setattr(pq.FaissIvfPq, "train", classmethod(fake_pq_train))
    monkeypatch.setattr(opq.FaissOpqIvfPq, "train", classmethod(fake_opq_train))
    monkeypatch.setattr(rf.FaissRefineFlat, "wrap", classmethod(fake_wrap))
    x = np.arange(40 * 32, dtype=np.float32).reshape(40, 32)
    out = rf.build_faiss_index(x, range(40), 0.25, "IVF2,PQ4,RFlat", m.L2, k_factor=8)
    assert isinstance(out, _Index)
    assert calls == [("train", "FaissIvfPq", m.L2, 2, 4, (10, 32), 0, 1), ("wrap", "_Base", 8), ("add", (40, 32), list(range(40)))]
    del calls[:]
    out = rf.build_faiss_index(x, range(40), 0.5, "OPQ4_16,IVF2,PQ4,Refine(Flat)", m.Cosine, k_factor=2, niter=3, niter_opq=5, seed=9)
    assert calls == [("train", "FaissOpqIvfPq", m.Cosine, 2, 4, 16, (20, 32), 3, 5, 9), ("wrap", "_Base", 2), ("add", (40, 32), list(range(40)))]
    del calls[:]
    out = rf.build_faiss_index(x, range(40), 0.25, "IVF2,PQ4", m.L2)
    assert isinstance(out, _Base), "a string without the suffix builds the plain index"
    assert calls == [("train", "FaissIvfPq", m.L2, 2, 4, (10, 32), 0, 1), ("base add", (40, 32), list(range(40)))]
    with pytest.raises(ValueError, match="RFlat "):
        rf.build_faiss_index(x, range(40), 0.25, "IVF2,PQ4,RFlat ", m.L2)


# ---- the hand-derived KAT: 2 queries, 6 rows, d = 4 ---------------------------------------------------------------------
ROWS = np.array([[1, 0, 0, 0],    # pos 0  id 50
                 [0, 1, 0, 0],    # pos 1  id 40
                 [1, 1, 0, 0],    # pos 2  id 30
                 [0, 1, 0, 0],    # pos 3  id 20: the row of pos 1 under a lower id -> a distance tie resolved by id
                 [2, 0, 0, 0],    # pos 4  id 10
                 [1, 0, 0, 0]],   # pos 5  id 50: the row AND the id of pos 0 -> a tie of both, resolved by position
                np.float32)
IDS = np.array([50, 40, 30, 20, 10, 50], np.int64)
QUERIES = np.array([[1, 0, 0, 0], [0, 2, 0, 0]], np.float32)
CANDIDATES = np.array([[5, 3, 1, 4, 2, 0], [1, 3, 2, -1, -1, -1]], np.int32)  # (in no useful order: the base's)
COUNTS = np.array([6, 3], np.int32)
H = 0.70703125  # 1 / sqrt 2 in fp16
KAT = {
    # query 0: ids, distances, positions, the 6th distance;  query 1 (3 candidates, k = 5): ids, distances, positions
    ref.L2: (([50, 50, 10, 30, 20], [0.0, 0.0, 1.0, 1.0, np.sqrt(2.0)], [0, 5, 4, 2, 3], np.sqrt(2.0)),
             ([20, 40, 30], [1.0, 1.0, np.sqrt(2.0)], [3, 1, 2])),
    # 1 - <q, x>
    ref.INNER_PRODUCT: (([10, 30, 50, 50, 20], [-1.0, 0.0, 0.0, 0.0, 1.0], [4, 2, 0, 5, 3], 1.0),
                        ([20, 30, 40], [-1.0, -1.0, -1.0], [3, 2, 1])),
    # rows and queries normalised first: (1, 1, 0, 0) -> (H, H, 0, 0), (2, 0, 0, 0) -> e0, (0, 2, 0, 0) -> e1
    ref.COSINE: (([10, 50, 50, 30, 20], [0.0, 0.0, 0.0, 1.0 - H, 1.0], [4, 0, 5, 2, 3], 1.0),
                 ([20, 40, 30], [0.0, 0.0, 1.0 - H], [3, 1, 2])),
}


@pytest.mark.parametrize("metric", [ref.L2, ref.INNER_PRODUCT, ref.COSINE])
def test_reference_rerank_by_hand(metric):
    rows, q = ref.prepare(metric, ROWS), ref.prepare(metric, QUERIES)
    got = ref.rerank(metric, rows, IDS, CANDIDATES, COUNTS, q, 5)
    (ids0, dist0, pos0, nxt0), (ids1, dist1, pos1) = KAT[metric]
    assert got[0][0].tolist() == ids0 and got[0][2].tolist() == pos0
    np.testing.assert_allclose(got[0][1], dist0, rtol=0, atol=1e-15)
    assert abs(got[0][3] - nxt0) <= 1e-15
    assert got[1][0].tolist() == ids1 and got[1][2].tolist() == pos1 and got[1][3] == np.inf
    np.testing.assert_allclose(got[1][1], dist1, rtol=0, atol=1e-15)
    # k below the count: the first k, the next distance is the (k+1)-th
    short = ref.rerank(metric, rows, IDS, CANDIDATES, COUNTS, q, 2)
    assert short[0][0].tolist() == ids0[:2] and abs(short[0][3] - dist0[2]) <= 1e-15
    assert short[1][0].tolist() == ids1[:2] and abs(short[1][3] - dist1[2]) <= 1e-15
    # no candidate at all
    none = ref.rerank(metric, rows, IDS, CANDIDATES, np.array([0, 0]), q, 2)
    assert len(none[0][0]) == 0 and none[0][3] == np.inf


def test_quality_input_orders_the_recalls_on_the_cpu():
    """The corpus of test_refine_gpu.py's quality test, checked by numpy alone (ADC by _ivfpq_ref.adc_search, then
    _refine_ref.rerank): mean recall@10 against the float64 exhaustive truth rises from plain ADC (k_factor = 1 keeps its
    set) over k_factor = 2 to k_factor = 8.  CPU values at QUALITY_SEED = 7: 0.2516, 0.4047, 0.8156."""
    p = QUALITY
    x, q = ref.quality_corpus(QUALITY_SEED, p["n"], p["d"], p["nq"])
    cent, cb = ref.numpy_train(ref.COSINE, x, p["nlist"], p["M"], QUALITY_SEED)
    got, truth = ref.cpu_refined(ref.COSINE, x, q, cent, cb, p["k"], (1, 2, 8), p["nprobe"])
    full = np.full(len(q), p["k"])
    r1, r2, r8 = (ref.recall(got[kf], full, truth) for kf in (1, 2, 8))
    print(f"CPU recall@10: plain ADC {r1:.4f}, k_factor 2 {r2:.4f}, k_factor 8 {r8:.4f}")
    assert r8 > r1 and r8 >= r2, (r1, r2, r8)
    assert r8 - r1 >= 0.05, "the margin the device test relies on"
