"""IVF-SQ8 (include/ivfsq_ann.h) without a GPU: the exported symbols, the refusals that come before any device call,
index_factory, and properties of the CPU restatement tests/_ivfsq_ref.py itself."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import _ivfsq_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1


@pytest.fixture(scope="module")
def sq(pkg):
    return importlib.import_module(pkg.__name__ + ".scalar_quantizer")


def test_library_exports_every_declared_symbol(pkg, sq):
    lib = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "ivfsq_ann.h")).read()
    declared = set(re.findall(r"\b(ivfsq_[a-z_0-9]+)\s*\(", header))
    assert len(declared) == 14, "declarations parsed"
    assert declared == set(sq.PROTOS)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/ivfsq_ann.h but not exported"


def test_package_does_not_reexport_the_subpackage_names(pkg, sq):
    for name in ("FaissIvfSq8", "Sq8IndexSpec", "IvfSqError"):
        assert not hasattr(pkg, name)
    assert sq.FaissIvfSq8.FAISS_KIND == 0
    assert issubclass(sq.FaissIvfSq8, pkg.ivf_ann._IvfFamilyIndex) and issubclass(sq.IvfSqError, pkg.ivf_ann.IvfError)


def test_argument_errors_return_before_any_device_call(sq):
    lib = sq._lib()
    h = C.c_void_p()
    x = np.zeros((300, 32), np.float32)
    ok = np.ones(528, np.float32)

    def err():
        return lib.ivfsq_last_error().decode()

    def train(metric=0, d=32, nlist=4, n=300, v=x.ctypes.data, niter=1, out=C.byref(h)):
        return lib.ivfsq_index_train(0, metric, d, nlist, n, v, niter, 1, out)

    def load(metric=0, d=32, nlist=4, c=x.ctypes.data, vmin=ok.ctypes.data, vdiff=ok.ctypes.data, out=C.byref(h)):
        return lib.ivfsq_index_load(0, metric, d, nlist, c, vmin, vdiff, out)

    for call in (train, load):
        assert call(d=24) == EINVAL and "multiple of 16" in err()
        assert call(d=528) == EINVAL and "multiple of 16" in err()
        assert call(d=0) == EINVAL
        assert call(nlist=0) == EINVAL and "nlist" in err()
        assert call(nlist=65537) == EINVAL and "nlist" in err()
        assert call(metric=7) == EINVAL and "metric" in err()
        assert call(out=None) == EINVAL and "null" in err()
    assert train(v=None) == EINVAL and "null" in err()
    assert train(nlist=301) == EINVAL and "n_train" in err()
    assert train(niter=-2) == EINVAL and "niter" in err()
    assert load(c=None) == EINVAL and "null" in err()
    assert load(vmin=None) == EINVAL and "null" in err()
    assert load(vdiff=None) == EINVAL and "null" in err()
    for bad, word in ((-1.0, "negative"), (np.nan, "finite"), (np.inf, "finite"), (-np.inf, "finite")):
        v = np.ones(32, np.float32)
        v[17] = bad
        assert load(vdiff=v.ctypes.data) == EINVAL and word in err() and "17" in err(), bad
    for bad in (np.nan, np.inf):
        v = np.zeros(32, np.float32)
        v[3] = bad
        assert load(vmin=v.ctypes.data) == EINVAL and "finite" in err()
    assert h.value is None
    assert lib.ivfsq_index_add(None, 1, x.ctypes.data, None) == EINVAL and "null" in err()
    out = np.zeros(64, np.int64)
    assert lib.ivfsq_search(None, 1, x.ctypes.data, 1, 1, out.ctypes.data, out.ctypes.data, out.ctypes.data) == EINVAL
    # k and nprobe are refused before the handle is looked at: any non-NULL pointer will do
    fake = C.create_string_buffer(8192)
    addr = C.addressof(fake)
    o = out.ctypes.data
    assert lib.ivfsq_search(addr, 1, x.ctypes.data, 1025, 1, o, o, o) == EINVAL and "k must" in err()
    assert lib.ivfsq_search(addr, 1, x.ctypes.data, 1, 0, o, o, o) == EINVAL and "nprobe" in err()
    assert lib.ivfsq_search(addr, 1, x.ctypes.data, 1, 1025, o, o, o) == EINVAL
    assert lib.ivfsq_search(addr, 0, x.ctypes.data, 1, 1, o, o, o) == EINVAL
    assert lib.ivfsq_search(addr, 1, None, 1, 1, o, o, o) == EINVAL and "null" in err()
    for fn in (lib.ivfsq_index_get_centroids, lib.ivfsq_index_list_sizes):
        assert fn(None, o) == EINVAL
    assert lib.ivfsq_index_get_ranges(None, o, o) == EINVAL
    assert lib.ivfsq_index_get_codes(None, 0, 0, o) == EINVAL
    assert lib.ivfsq_index_get_codes(addr, 0, 0, None) == EINVAL
    assert lib.ivfsq_index_info(None, None, None, None, None) == EINVAL
    assert lib.ivfsq_index_get_assignment(None, None, None) == EINVAL
    assert lib.ivfsq_last_probes(None, None, None, None) == EINVAL
    assert lib.ivfsq_last_stats(None, None, None, None, None, None) == EINVAL
    assert lib.ivfsq_index_destroy(None) == 0
    # ranges of the wrong length never reach the library
    with pytest.raises(ValueError, match="vmin"):
        sq.FaissIvfSq8.load(0, np.zeros((2, 16), np.float32), np.zeros(15, np.float32), np.zeros(16, np.float32))


def test_index_factory_strings(pkg, sq):
    m = pkg.dense_ann.DistanceMetric
    spec = sq.index_factory(64, "IVF64,SQ8", m.Cosine)
    assert isinstance(spec, sq.Sq8IndexSpec) and spec.index_class is sq.FaissIvfSq8
    assert (spec.nlist, spec.dimension, spec.metric, spec.factory_string, spec.M) == (64, 64, m.Cosine, "IVF64,SQ8", None)
    for bad in ["IVF64,SQ4", "IVF64,SQ6", "IVF64,SQfp16", "IVF64,SQ8,RFlat", "IVF64_HNSW32,SQ8", "SQ8", "IVF,SQ8", "ivf64,sq8",
                "IVF64,SQ8 ", None]:
        with pytest.raises(ValueError) as e:
            sq.index_factory(64, bad, m.L2)
        assert repr(bad) in str(e.value), "the message names the string"
    # every other string reaches the older factories
    spec = sq.index_factory(64, "IVF64,PQ8", m.L2)
    assert type(spec) is pkg.ivfpq_ann.IndexSpec and (spec.nlist, spec.M) == (64, 8)
    assert sq.index_factory(64, "IVF64,Flat", m.L2).index_class is pkg.ivf_ann.FaissIvfFlat
    assert type(sq.index_factory(64, "IVF64_HNSW32,Flat", m.L2)).__name__ == "HnswQuantizedIndexSpec"
    assert type(sq.index_factory(64, "OPQ16,IVF64,PQ16", m.L2)).__name__ == "OpqIndexSpec"


def test_build_trains_on_the_head_and_adds_all(pkg, sq, monkeypatch):
    calls = []

    class _Index:
        def add(self, v, ids):
            calls.append(("add", v.shape, list(ids)))

    def fake_train(cls, metric, nlist, v, *, niter, seed, device):
        calls.append(("train", cls.__name__, metric, nlist, v.shape, niter, seed, device))
        return _Index()

    monkeypatch.setattr(sq.FaissIvfSq8, "train", classmethod(fake_train))
    m = pkg.dense_ann.DistanceMetric
    x = np.arange(40 * 16, dtype=np.float32).reshape(40, 16)
    out = sq.build_faiss_index(x, range(40), 0.25, "IVF2,SQ8", m.L2, niter=3, seed=9)
    assert isinstance(out, _Index)
    assert calls == [("train", "FaissIvfSq8", m.L2, 2, (10, 16), 3, 9, 0), ("add", (40, 16), list(range(40)))]
    with pytest.raises(ValueError, match="IVF2,SQ4"):
        sq.build_faiss_index(x, range(40), 0.25, "IVF2,SQ4", m.L2)


def test_queryable_works_over_the_index_as_it_is(pkg, sq):
    class _Stub(sq.FaissIvfSq8):
        def __init__(self):
            self._h = None

        def search(self, q, k, nprobe):
            assert nprobe == 7 and k == 2
            return np.array([[5, 9]], np.int64), np.array([[0.25, 1.5]], np.float32), np.array([2], np.int32)

    qa = pkg.ivf_ann.FaissQueryable(_Stub(), pkg.dense_ann.DistanceMetric.Cosine)
    got = qa.queryWithDistance(np.zeros(16, np.float32), 2, pkg.ivf_ann.FaissParams(nprobe=7))
    assert got == [(5, 0.25), (9, 1.0)], "Cosine: a similarity outside [0, 1] becomes the maximal distance"


# ---- the restatement itself ---------------------------------------------------------------------------------------------
def live_cols(step):
    return np.flatnonzero(step > 0)


def test_reference_known_codes_by_hand():
    vmin, vdiff = np.zeros(16, np.float32), np.full(16, 255, np.float32)
    assert ref.step_of(vdiff).tolist() == [1.0] * 16
    x = np.zeros((5, 16), np.float32)
    x[:, 2] = [0.5, 3.7, 254.9, 300.0, -4.0]
    x = ref.prepare(ref.INNER_PRODUCT, x)
    codes = ref.encode(x, vmin, vdiff)
    assert codes[:, 2].tolist() == [0, 3, 254, 255, 0] and not codes[:, :2].any() and not codes[:, 3:].any()
    q = np.zeros((1, 16), np.float32)
    q[0, 2] = 1.0
    assert ref.b_q(q, vmin, vdiff).tolist() == [0.5]
    assert ref.inner_products(q, codes, vmin, vdiff)[0].tolist() == [0.5, 3.5, 254.5, 255.5, 0.5]
    assert ref.distances(ref.INNER_PRODUCT, q, codes, vmin, vdiff)[0].tolist() == [0.5, -2.5, -253.5, -254.5, 0.5]
    # L2: |xhat|^2 = 15 * 0.25 + (c + 0.5)^2, |q|^2 = 1
    d2 = ref.distances(ref.L2, q, codes, vmin, vdiff)[0] ** 2
    np.testing.assert_allclose(d2[:2], [1 - 2 * 0.5 + 15 * 0.25 + 0.25, 1 - 2 * 3.5 + 15 * 0.25 + 12.25], rtol=1e-12)


def test_reference_quantisation_properties():
    rng = np.random.default_rng(3)
    d = 48
    train = ref.prepare(ref.L2, rng.standard_normal((500, d)) * rng.uniform(0.01, 30, d))
    train[:, 7] = np.float32(0.375)  # a constant component
    train[:, 8] = 0.0
    train[::2, 8] = -0.0
    vmin, vdiff = ref.ranges(train)
    step = ref.step_of(vdiff)
    assert vmin.dtype == np.float32 and vdiff.dtype == np.float32 and step.dtype == np.float32
    assert vdiff[7] == 0 and step[7] == 0 and vmin[7] == np.float32(0.375)
    assert vdiff[8] == 0 and not np.signbit(vmin[8]), "a zero minimum is +0"
    assert np.array_equal(ref.ranges(train[::-1])[0], vmin) and np.array_equal(ref.ranges(train[rng.permutation(500)])[1], vdiff)
    # inside the range: |x - xhat| <= step / 2 (up to the fp32 roundings of the subtraction and the division)
    codes = ref.encode(train, vmin, vdiff)
    assert codes.dtype == np.uint8 and not codes[:, 7].any() and not codes[:, 8].any()
    err = np.abs(train.astype(np.float64) - ref.xhat(codes, vmin, vdiff))
    slack = 0.5 * step.astype(np.float64) * (1 + 2.0 ** -14)
    assert (err <= slack[None, :]).all()
    assert err[:, 7].max() == 0, "a constant component is stored exactly: vmin + 0.5 * 0"
    # the extremes of the training set take the end codes (the maximum 254 where fl32(vdiff / step) falls just below 255)
    assert (codes[:, live_cols(step)].min(axis=0) == 0).all() and (codes[:, live_cols(step)].max(axis=0) >= 254).all()
    # outside: clipping, both ways
    far = np.stack([vmin - 3 * vdiff - 1, vmin + 4 * vdiff + 1]).astype(np.float16).astype(np.float32)
    cfar = ref.encode(far, vmin, vdiff)
    live = step > 0
    assert not cfar[0].any() and (cfar[1][live] == 255).all() and not cfar[1][~live].any()
    # the scaled query is a float16 value, b_q a float32 value
    q = ref.prepare(ref.L2, rng.standard_normal((4, d)))
    s = ref.scaled_queries(q, vdiff)
    assert np.array_equal(s, s.astype(np.float16).astype(np.float64))
    b = ref.b_q(q, vmin, vdiff)
    assert np.array_equal(b, b.astype(np.float32).astype(np.float64))
    # P is close to <q, xhat>: the only difference is the rounding of s (2^-11 relative per term) and of b_q
    exact = q.astype(np.float64) @ ref.xhat(codes, vmin, vdiff).T
    bound = (np.abs(q.astype(np.float64)) * step[None, :]).sum(axis=1) * 255 * 2.0 ** -11 + np.abs(b) * 2.0 ** -23
    assert (np.abs(ref.inner_products(q, codes, vmin, vdiff) - exact) <= bound[:, None]).all()


def test_reference_search_probed_orders_by_distance_then_id():
    dist = np.array([[3.0, 1.0, 1.0, 2.0, 0.5]])
    ids = np.array([10, 9, 4, 7, 1])
    cells = np.array([0, 0, 0, 1, 2])
    (r_ids, r_dist, nxt), = ref.search_probed(dist, ids, cells, np.array([[0, 1]]), 3)
    assert r_ids.tolist() == [4, 9, 7] and r_dist.tolist() == [1.0, 1.0, 2.0] and nxt == 3.0
    (r_ids, r_dist, nxt), = ref.search_probed(dist, ids, cells, np.array([[2]]), 3)
    assert r_ids.tolist() == [1] and nxt == np.inf
