"""IVF-Flat (include/ivf_ann.h) without a GPU: the exported symbols, argument errors that return before any device call,
the CPU restatement tests/_ivf_ref.py against hand-derived answers, and FaissQueryable with the search stubbed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _ivf_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1


def test_library_exports_every_declared_symbol(pkg):
    lib = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "ivf_ann.h")).read()
    declared = set(re.findall(r"\b(ivf_[a-z_0-9]+)\s*\(", header))
    assert len(declared) >= 12, "declarations parsed"
    assert declared == set(pkg.ivf_ann.PROTOS)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/ivf_ann.h but not exported"


def test_argument_errors_return_before_any_device_call(pkg):
    lib = pkg.ivf_ann._lib()
    h = C.c_void_p()
    x = np.zeros((8, 32), np.float32)

    def err():
        return lib.ivf_last_error().decode()

    assert lib.ivf_index_train(0, 0, 24, 4, 8, x.ctypes.data, 1, 1, C.byref(h)) == EINVAL and "multiple of 16" in err()
    assert lib.ivf_index_train(0, 0, 32, 0, 8, x.ctypes.data, 1, 1, C.byref(h)) == EINVAL and "nlist" in err()
    assert lib.ivf_index_train(0, 0, 32, 9, 8, x.ctypes.data, 1, 1, C.byref(h)) == EINVAL and "n_train" in err()
    assert lib.ivf_index_train(0, 0, 32, 4, 8, None, 1, 1, C.byref(h)) == EINVAL and "null" in err()
    assert lib.ivf_index_train(0, 0, 32, 4, 8, x.ctypes.data, 1, 1, None) == EINVAL
    assert lib.ivf_index_train(0, 7, 32, 4, 8, x.ctypes.data, 1, 1, C.byref(h)) == EINVAL and "metric" in err()
    assert lib.ivf_index_train(0, 0, 32, 4, 8, x.ctypes.data, -2, 1, C.byref(h)) == EINVAL and "niter" in err()
    assert lib.ivf_index_load(0, 0, 32, 4, None, C.byref(h)) == EINVAL and "null" in err()
    assert lib.ivf_index_load(0, 0, 528, 4, x.ctypes.data, C.byref(h)) == EINVAL
    assert lib.ivf_index_load(0, 0, 32, 65537, x.ctypes.data, C.byref(h)) == EINVAL
    assert h.value is None
    assert lib.ivf_index_add(None, 1, x.ctypes.data, None) == EINVAL and "null" in err()
    out = np.zeros(64, np.int64)
    assert lib.ivf_search(None, 1, x.ctypes.data, 1, 1, out.ctypes.data, out.ctypes.data, out.ctypes.data) == EINVAL
    # k and nprobe are refused before the handle is looked at: any non-NULL pointer will do
    fake = C.create_string_buffer(4096)
    addr = C.addressof(fake)
    assert lib.ivf_search(addr, 1, x.ctypes.data, 1025, 1, out.ctypes.data, out.ctypes.data, out.ctypes.data) == EINVAL and "k must" in err()
    assert lib.ivf_search(addr, 1, x.ctypes.data, 1, 0, out.ctypes.data, out.ctypes.data, out.ctypes.data) == EINVAL and "nprobe" in err()
    assert lib.ivf_search(addr, 1, x.ctypes.data, 1, 1025, out.ctypes.data, out.ctypes.data, out.ctypes.data) == EINVAL
    assert lib.ivf_search(addr, 0, x.ctypes.data, 1, 1, out.ctypes.data, out.ctypes.data, out.ctypes.data) == EINVAL
    assert lib.ivf_search(addr, 1, None, 1, 1, out.ctypes.data, out.ctypes.data, out.ctypes.data) == EINVAL
    for fn in (lib.ivf_index_get_centroids, lib.ivf_index_list_sizes):
        assert fn(None, out.ctypes.data) == EINVAL
    assert lib.ivf_index_info(None, None, None, None, None) == EINVAL
    assert lib.ivf_index_get_assignment(None, None, None) == EINVAL
    assert lib.ivf_last_probes(None, None, None, None) == EINVAL
    assert lib.ivf_last_stats(None, None, None, None, None, None) == EINVAL
    assert lib.ivf_index_destroy(None) == 0


def _axis(*pairs):
    v = np.zeros(16, np.float32)
    for k, a in pairs:
        v[k] = a
    return v


# four centroids on coordinate axes and a dozen rows (every value exact in fp16); cell 3 stays empty
CENTROIDS = np.stack([_axis((c, 1.0)) for c in range(4)])
ROWS = np.stack([
    _axis((0, 1.0)),             # id 10  cell 0
    _axis((0, 1.0)),             # id 5   cell 0, a duplicate of id 10
    _axis((0, 0.75), (1, 0.25)), # id 7   cell 0
    _axis((1, 1.0)),             # id 20  cell 1
    _axis((1, 0.5), (2, 0.25)),  # id 21  cell 1
    _axis((2, 1.0)),             # id 30  cell 2
    _axis((1, 0.75), (0, 0.5)),  # id 22  cell 1
    _axis((2, 0.5)),             # id 31  cell 2
    _axis((0, 0.25), (2, 0.5)),  # id 32  cell 2
    _axis((0, 0.5), (1, 0.5)),   # id 1   cells 0 and 1 tie in every metric: the lower cell
    _axis((1, 0.75)),            # id 23  cell 1
    _axis((0, 0.25)),            # id 2   cell 0
])
IDS = np.array([10, 5, 7, 20, 21, 30, 22, 31, 32, 1, 23, 2], np.int64)
CELLS = [0, 0, 0, 1, 1, 2, 1, 2, 2, 0, 1, 0]
Q = np.stack([_axis((0, 1.0), (1, 0.5)), _axis((3, 1.0))])


@pytest.mark.parametrize("metric", [ref.L2, ref.COSINE, ref.INNER_PRODUCT])
def test_reference_assignment_and_probes(metric):
    ix = ref.IvfRef(metric, CENTROIDS)
    ix.add(ROWS[:7], IDS[:7])
    ix.add(ROWS[7:], IDS[7:])
    assert ix.cells.tolist() == CELLS
    assert ix.list_sizes().tolist() == [5, 4, 3, 0]
    _, _, cnt, probes = ix.search(Q, 3, 1)
    assert probes.tolist() == [[0], [3]]
    assert cnt.tolist() == [3, 0], "the second query probes the empty cell"
    _, _, cnt, probes = ix.search(Q, 8, 2)
    # query 1: e3's own cell, then cells 0..2 tie (L2 sqrt 2 each, dot 0 each): the lower cell
    assert probes.tolist() == [[0, 1], [3, 0]]
    assert cnt.tolist() == [8, 5], "lists shorter than k: counts fall short"
    _, _, _, probes = ix.search(Q, 1, 9)
    assert probes.shape == (2, 4), "nprobe above nlist is clamped"
    with pytest.raises(ValueError):
        ix.add(ROWS[:1])


def test_reference_answers_by_hand():
    q = Q[:1]
    # InnerProduct, cell 0 alone: dots 1, 1, 0.875, 0.75, 0.25 for ids 10, 5, 7, 1, 2 -> ties by id
    ix = ref.IvfRef(ref.INNER_PRODUCT, CENTROIDS)
    ix.add(ROWS, IDS)
    ids, dist, cnt, _ = ix.search(q, 3, 1)
    assert ids[0].tolist() == [5, 10, 7] and dist[0].tolist() == [0.0, 0.0, 0.125]
    ids, dist, cnt, _ = ix.search(q, 8, 1)
    assert cnt[0] == 5 and ids[0, :5].tolist() == [5, 10, 7, 1, 2]
    assert dist[0, :5].tolist() == [0.0, 0.0, 0.125, 0.25, 0.75]
    # two cells: id 22 = (0.5, 0.75) has dot 0.875 too and ties with id 7
    ids, dist, cnt, _ = ix.search(q, 4, 2)
    assert ids[0].tolist() == [5, 10, 7, 22]
    # L2, cell 0: id 7 at sqrt(1/8), then ids 1, 5, 10 all at 0.5, id 2 at sqrt(13)/4
    ix = ref.IvfRef(ref.L2, CENTROIDS)
    ix.add(ROWS, IDS)
    ids, dist, cnt, _ = ix.search(q, 3, 1)
    assert ids[0].tolist() == [7, 1, 5]
    np.testing.assert_allclose(dist[0], [np.sqrt(0.125), 0.5, 0.5], rtol=1e-12)
    ids, dist, cnt, _ = ix.search(q, 8, 1)
    assert cnt[0] == 5 and ids[0, :5].tolist() == [7, 1, 5, 10, 2]
    np.testing.assert_allclose(dist[0, 4], np.sqrt(13.0) / 4, rtol=1e-12)
    # Cosine: ids 5, 10 and 2 point along e0 and tie (cos 2 / sqrt 5); id 7 is nearest, then id 1
    ix = ref.IvfRef(ref.COSINE, CENTROIDS)
    ix.add(ROWS, IDS)
    ids, dist, cnt, _ = ix.search(q, 5, 1)
    assert ids[0].tolist() == [7, 1, 2, 5, 10]
    np.testing.assert_allclose(dist[0, 2:], 1 - 2 / np.sqrt(5.0), atol=2e-3)  # (fp16 rounding of the unit vectors)
    assert dist[0, 2] == dist[0, 3] == dist[0, 4]


def test_clear_positions():
    assert ref.clear_positions([0.0, 1.0, 1.0, 2.0], np.inf).tolist() == [True, False, False, True]
    assert ref.clear_positions([0.0, 1.0], 1.0).tolist() == [True, False]
    assert ref.clear_positions([], np.inf).tolist() == []


class _Stub:
    def __init__(self, dist):
        self.dist, self.calls = np.asarray(dist, np.float32), []

    def search(self, q, k, nprobe):
        self.calls.append((k, nprobe))
        m = len(self.dist)
        return np.arange(100, 100 + m)[None, :], self.dist[None, :], np.array([m], np.int32)


def test_faiss_queryable_cosine_clamp_and_parameters(pkg):
    iv = pkg.ivf_ann
    m = pkg.dense_ann.DistanceMetric
    # similarities 1.25 (outside), 0.75, 0 and -0.5 (outside): distance 1 for the two outside, order as returned
    stub = _Stub([-0.25, 0.25, 1.0, 1.5])
    got = iv.FaissQueryable(stub, m.Cosine).queryWithDistance(np.zeros(16), 4, iv.FaissParams(nprobe=3))
    assert got == [(100, 1.0), (101, 0.25), (102, 1.0), (103, 1.0)]
    assert stub.calls == [(4, 3)]
    # other metrics pass through
    got = iv.FaissQueryable(stub, m.InnerProduct).queryWithDistance(np.zeros(16), 4, iv.FaissParams(nprobe=1))
    assert [d for _, d in got] == [-0.25, 0.25, 1.0, 1.5]
    assert iv.FaissQueryable(stub, m.L2).query(np.zeros(16), 4, iv.FaissParams(nprobe=1)) == [100, 101, 102, 103]
    for field in ("quantizerEf", "quantizerKfactorRf", "quantizerNprobe", "ht"):
        with pytest.raises(ValueError, match=field):
            iv.FaissQueryable(stub, m.L2).queryWithDistance(np.zeros(16), 4, iv.FaissParams(nprobe=1, **{field: 2}))
    with pytest.raises(ValueError, match="nprobe"):
        iv.FaissQueryable(stub, m.L2).queryWithDistance(np.zeros(16), 4, iv.FaissParams())
