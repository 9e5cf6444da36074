"""IVF-PQ (include/ivfpq_ann.h) without a GPU: the exported symbols, argument errors that return before any device call,
the CPU restatement tests/_ivfpq_ref.py against answers derived by hand, index_factory and the training-set size."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _ivfpq_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1


def test_library_exports_every_declared_symbol(pkg):
    lib = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "ivfpq_ann.h")).read()
    declared = set(re.findall(r"\b(ivfpq_[a-z_0-9]+)\s*\(", header))
    assert len(declared) >= 14, "declarations parsed"
    assert declared == set(pkg.ivfpq_ann.PROTOS)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/ivfpq_ann.h but not exported"


def test_argument_errors_return_before_any_device_call(pkg):
    lib = pkg.ivfpq_ann._lib()
    h = C.c_void_p()
    x = np.zeros((300, 32), np.float32)

    def err():
        return lib.ivfpq_last_error().decode()

    def train(metric=0, d=32, nlist=4, M=8, n=300, v=x.ctypes.data, niter=1, out=C.byref(h)):
        return lib.ivfpq_index_train(0, metric, d, nlist, M, n, v, niter, 1, out)

    assert train(d=24) == EINVAL and "multiple of 16" in err()
    assert train(nlist=0) == EINVAL and "nlist" in err()
    assert train(M=12) == EINVAL and "divide" in err(), "M does not divide d"
    assert train(M=6) == EINVAL and "multiple of 4" in err()
    assert train(M=2) == EINVAL and "multiple of 4" in err()
    assert lib.ivfpq_index_train(0, 0, 512, 4, 128, 300, x.ctypes.data, 1, 1, C.byref(h)) == EINVAL and "4..64" in err()
    assert train(n=255) == EINVAL and "n_train" in err(), "fewer training rows than codewords"
    assert train(nlist=301) == EINVAL and "n_train" in err()
    assert train(v=None) == EINVAL and "null" in err()
    assert train(out=None) == EINVAL
    assert train(metric=7) == EINVAL and "metric" in err()
    assert train(niter=-2) == EINVAL and "niter" in err()
    assert lib.ivfpq_index_load(0, 0, 32, 4, 8, None, x.ctypes.data, C.byref(h)) == EINVAL and "null" in err()
    assert lib.ivfpq_index_load(0, 0, 32, 4, 8, x.ctypes.data, None, C.byref(h)) == EINVAL and "null" in err()
    assert lib.ivfpq_index_load(0, 0, 528, 4, 8, x.ctypes.data, x.ctypes.data, C.byref(h)) == EINVAL
    assert lib.ivfpq_index_load(0, 0, 32, 65537, 8, x.ctypes.data, x.ctypes.data, C.byref(h)) == EINVAL
    assert lib.ivfpq_index_load(0, 0, 32, 4, 5, x.ctypes.data, x.ctypes.data, C.byref(h)) == EINVAL
    assert h.value is None
    assert lib.ivfpq_index_add(None, 1, x.ctypes.data, None) == EINVAL and "null" in err()
    out = np.zeros(64, np.int64)
    assert lib.ivfpq_search(None, 1, x.ctypes.data, 1, 1, out.ctypes.data, out.ctypes.data, out.ctypes.data) == EINVAL
    # k and nprobe are refused before the handle is looked at: any non-NULL pointer will do
    fake = C.create_string_buffer(4096)
    addr = C.addressof(fake)
    assert lib.ivfpq_search(addr, 1, x.ctypes.data, 1025, 1, out.ctypes.data, out.ctypes.data, out.ctypes.data) == EINVAL and "k must" in err()
    assert lib.ivfpq_search(addr, 1, x.ctypes.data, 1, 0, out.ctypes.data, out.ctypes.data, out.ctypes.data) == EINVAL and "nprobe" in err()
    assert lib.ivfpq_search(addr, 1, x.ctypes.data, 1, 1025, out.ctypes.data, out.ctypes.data, out.ctypes.data) == EINVAL
    assert lib.ivfpq_search(addr, 0, x.ctypes.data, 1, 1, out.ctypes.data, out.ctypes.data, out.ctypes.data) == EINVAL
    for fn in (lib.ivfpq_index_get_centroids, lib.ivfpq_index_list_sizes, lib.ivfpq_index_get_codebooks, lib.ivfpq_index_get_codes):
        assert fn(None, out.ctypes.data) == EINVAL
    assert lib.ivfpq_index_info(None, None, None, None, None, None) == EINVAL
    assert lib.ivfpq_index_get_assignment(None, None, None) == EINVAL
    assert lib.ivfpq_last_probes(None, None, None, None) == EINVAL
    assert lib.ivfpq_last_stats(None, None, None, None, None, None) == EINVAL
    assert lib.ivfpq_index_destroy(None) == 0
    # a codebook of the wrong length never reaches the library
    with pytest.raises(ValueError, match="codebooks"):
        pkg.ivfpq_ann.FaissIvfPq.load(pkg.dense_ann.DistanceMetric.L2, np.zeros((2, 16), np.float32), np.zeros((4, 256, 8), np.float32))
    with pytest.raises(ValueError, match="codebooks"):
        pkg.ivfpq_ann.FaissIvfPq.load(pkg.dense_ann.DistanceMetric.L2, np.zeros((2, 16), np.float32), np.zeros((4, 255, 4), np.float32))


# ---- the hand-derived KAT: d = 16, M = 4 (dsub = 4), nlist = 2 --------------------------------------------------------
# Codeword j of every subspace is (j / 8, 0, 0, 0); the centroids are e0 and e4.  Every value is exact in fp16.
def _vec(*pairs):
    v = np.zeros(16, np.float32)
    for k, a in pairs:
        v[k] = a
    return v


CODEBOOKS = np.zeros((4, 256, 4), np.float32)
CODEBOOKS[:, :, 0] = np.arange(256) / 8.0
CENTROIDS = np.stack([_vec((0, 1.0)), _vec((4, 1.0))])
ROWS = np.stack([
    _vec((0, 2.0), (8, 2.0)),       # id 30  cell 0: r = (1 | 0 | 2 | 0)            codes 8, 0, 16, 0
    _vec((4, 1.5), (12, 0.25)),     # id 5   cell 1: r = (0 | 0.5 | 0 | 0.25)       codes 0, 4, 0, 2
    _vec((0, 1.0625), (8, -1.0)),   # id 20  cell 0: r = (1/16 | 0 | -1 | 0): 1/16 is halfway between codewords 0 and 1 ->
                                    #        the lower; -1 is nearest codeword 0    codes 0, 0, 0, 0
    _vec((0, 1.375), (1, 0.5)),     # id 10  cell 0: r = (0.375, 0.5 | 0 | 0 | 0)   codes 3, 0, 0, 0
    _vec((0, 2.0), (8, 2.0)),       # id 7   a duplicate of id 30
])
IDS = np.array([30, 5, 20, 10, 7], np.int64)
CELLS = [0, 1, 0, 0, 0]
CODES = [[8, 0, 16, 0], [0, 4, 0, 2], [0, 0, 0, 0], [3, 0, 0, 0], [8, 0, 16, 0]]
Q = _vec((0, 2.0), (4, 1.0), (8, 1.0))[None, :]


@pytest.mark.parametrize("metric", [ref.L2, ref.INNER_PRODUCT])
def test_reference_encoding_by_hand(metric):
    ix = ref.IvfPqRef(metric, CENTROIDS, CODEBOOKS)
    ix.add(ROWS[:2], IDS[:2])
    ix.add(ROWS[2:], IDS[2:])
    assert ix.cells.tolist() == CELLS
    assert ix.codes.tolist() == CODES
    with pytest.raises(ValueError):
        ix.add(ROWS[:1])


def test_reference_answers_by_hand():
    # L2: cell 0 is nearer (3 against 5).  u = q - e0 = (1 | 1 | 1 | 0), first components of the subspaces.
    #   ids 7, 30: (1-1)^2 + 1 + (1-2)^2 = 2;  id 10: (1-0.375)^2 + 1 + 1 = 2.390625;  id 20: 1 + 1 + 1 = 3
    ix = ref.IvfPqRef(ref.L2, CENTROIDS, CODEBOOKS)
    ix.add(ROWS, IDS)
    ids, dist, cnt, probes = ix.search(Q, 3, 1)
    assert probes.tolist() == [[0]] and cnt.tolist() == [3]
    assert ids[0].tolist() == [7, 30, 10]
    np.testing.assert_allclose(dist[0], [np.sqrt(2.0), np.sqrt(2.0), np.sqrt(2.390625)], rtol=1e-15)
    ids, dist, cnt, probes = ix.search(Q, 8, 2)
    #   cell 1: u = q - e4 = (2 | 0 | 1 | 0); id 5: 4 + 0.25 + 1 + 0.0625 = 5.3125
    assert probes.tolist() == [[0, 1]] and cnt.tolist() == [5]
    assert ids[0, :5].tolist() == [7, 30, 10, 20, 5]
    np.testing.assert_allclose(dist[0, 3:5], [np.sqrt(3.0), np.sqrt(5.3125)], rtol=1e-15)
    # InnerProduct: <q, e0> = 2, <q, e4> = 1.  sim: ids 7, 30: 2 + 2*1 + 1*2 = 6;  id 10: 2 + 2*0.375 = 2.75;  id 20: 2;
    #   id 5: 1 + 1*0.5 = 1.5
    ix = ref.IvfPqRef(ref.INNER_PRODUCT, CENTROIDS, CODEBOOKS)
    ix.add(ROWS, IDS)
    ids, dist, cnt, probes = ix.search(Q, 8, 9)
    assert probes.tolist() == [[0, 1]], "nprobe above nlist is clamped"
    assert cnt.tolist() == [5] and ids[0, :5].tolist() == [7, 30, 10, 20, 5]
    assert dist[0, :5].tolist() == [-5.0, -5.0, -1.75, -1.0, -0.5]
    # Cosine: rows and queries are normalised first.  3 e0 -> e0: cell 0, residual 0, codes 0, similarity to q = 5 e0 is
    # <e0, e0> + 0 = 1; 2 e4 -> e4: cell 1, similarity <e0, e4> + 0 = 0; 2 e0 + 2 e8 -> (e0 + e8) / sqrt 2 in fp16 =
    # 0.70703125 each: cell 0, r = (-0.29296875 | 0 | 0.70703125 | 0) -> codes 0, 0, 6 (0.75 is nearer than 0.625), 0,
    # similarity 1 + 0 = 1 again: a tie with the first row, the lower id first
    ix = ref.IvfPqRef(ref.COSINE, CENTROIDS, CODEBOOKS)
    ix.add(np.stack([_vec((0, 3.0)), _vec((4, 2.0)), _vec((0, 2.0), (8, 2.0))]), [9, 8, 3])
    assert ix.cells.tolist() == [0, 1, 0]
    assert ix.codes.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 6, 0]]
    ids, dist, cnt, _ = ix.search(_vec((0, 5.0))[None, :], 3, 2)
    assert cnt.tolist() == [3] and ids[0].tolist() == [3, 9, 8] and dist[0].tolist() == [0.0, 0.0, 1.0]


def test_tolerance_and_clear_positions():
    # (M + dsub + d + 4) 2^-24 per unit of S on top of the project's 1e-5 / 1e-5; L2 has 2^-22 s more
    assert ref.fp32_bound(8, 8) == (8 + 8 + 64 + 4) * 2.0 ** -24
    assert ref.tolerance(ref.INNER_PRODUCT, -1.0, 4.0, 8, 8) == 1e-5 + 1e-5 + 4.0 * ref.fp32_bound(8, 8)
    assert ref.tolerance(ref.L2, 2.0, 2.0, 8, 8) == 1e-5 + 2e-5 + 2.0 * ref.fp32_bound(8, 8) + 2.0 * 2.0 ** -22
    tol = np.full(4, 1e-5)
    assert ref.clear_positions([0.0, 1.0, 1.0, 2.0], np.inf, tol).tolist() == [True, False, False, True]
    assert ref.clear_positions([0.0, 1.0], 1.0, tol[:2]).tolist() == [True, False]
    assert ref.clear_positions([0.0, 1.0], 1.5, np.array([1e-5, 0.3])).tolist() == [True, False]
    assert ref.clear_positions([], np.inf, tol[:0]).tolist() == []


def test_index_factory_strings(pkg):
    pq = pkg.ivfpq_ann
    m = pkg.dense_ann.DistanceMetric
    spec = pq.index_factory(64, "IVF1024,Flat", m.L2)
    assert (spec.nlist, spec.M, spec.dimension, spec.metric) == (1024, None, 64, m.L2) and spec.index_class is pkg.ivf_ann.FaissIvfFlat
    spec = pq.index_factory(256, "IVF4096,PQ32", m.Cosine)
    assert (spec.nlist, spec.M) == (4096, 32) and spec.index_class is pq.FaissIvfPq
    spec = pq.index_factory(256, "IVF16,PQ64x8", m.InnerProduct)
    assert (spec.nlist, spec.M) == (16, 64)
    for bad in ["", "Flat", "IVF,PQ8", "IVF64", "IVF64,PQ", "IVF64,PQ8x4", "IVF64,PQ8x16", "OPQ16,IVF64,PQ16", "IVF64_HNSW32,PQ8",
                "IVF64,PQ8,RFlat", "IVF64,SQ8", "ivf64,pq8", " IVF64,PQ8", "IVF64, PQ8", "HNSW32", None]:
        with pytest.raises(ValueError) as e:
            pq.index_factory(64, bad, m.L2)
        assert repr(bad) in str(e.value), "the message names the string"


def test_training_set_size_and_build(pkg, monkeypatch):
    pq = pkg.ivfpq_ann
    m = pkg.dense_ann.DistanceMetric
    # FaissIndexer.scala:86: min(n, round(n * sampleRate)), the product in Float, rounded half up
    assert pq.training_set_size(1000, 0.1) == 100
    assert pq.training_set_size(1000, 1.0) == 1000
    assert pq.training_set_size(1000, 2.5) == 1000
    assert pq.training_set_size(5, 0.5) == 3, "2.5 rounds up"
    assert pq.training_set_size(7, 0.5) == 4
    assert pq.training_set_size(1000, 0.0) == 0
    calls = []

    class _Index:
        def add(self, v, ids):
            calls.append(("add", v.shape, list(ids)))

    def fake_train(cls, metric, nlist, M, v, *, niter, seed, device):
        calls.append(("train", cls.__name__, metric, nlist, M, v.shape, niter, seed))
        return _Index()

    monkeypatch.setattr(pq.FaissIvfPq, "train", classmethod(fake_train))
    x = np.arange(40 * 16, dtype=np.float32).reshape(40, 16)
    out = pq.build_faiss_index(x, range(40), 0.25, "IVF2,PQ4", m.L2)
    assert isinstance(out, _Index)
    assert calls[0] == ("train", "FaissIvfPq", m.L2, 2, 4, (10, 16), 0, 1), "the first trainingSetSize rows"
    assert calls[1] == ("add", (40, 16), list(range(40))), "all rows are added"
    with pytest.raises(ValueError, match="IVF2,PQ4x2"):
        pq.build_faiss_index(x, range(40), 0.25, "IVF2,PQ4x2", m.L2)
