"""Ownership of real handles through binding.Handle: a wrapped base, an adopted index, an index made from a loaded handle.
The smallest shapes the library admits; every step is a call sequence a caller may make."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, D_IN, M, NLIST, N_TRAIN, N, NQ, K, NPROBE = 16, 32, 4, 4, 256, 64, 3, 4, 4


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(5)
    return {16: rng.standard_normal((N_TRAIN, D)).astype(np.float32), 32: rng.standard_normal((N_TRAIN, D_IN)).astype(np.float32),
            "ids": np.arange(1000, 1000 + N, dtype=np.int64)}


def _trained(pkg, kind, data):
    m = pkg.dense_ann.DistanceMetric.L2
    if kind == "flat":
        return pkg.ivf_ann.FaissIvfFlat.train(m, NLIST, data[16], niter=-1)
    if kind == "pq":
        return pkg.ivfpq_ann.FaissIvfPq.train(m, NLIST, M, data[16], niter=-1)
    return pkg.opq_ann.FaissOpqIvfPq.train(m, NLIST, M, D, data[32], niter=-1, niter_opq=1)


def _rows(kind, data):
    return data[32 if kind == "opq" else 16]


@pytest.mark.parametrize("kind", ["pq", "opq"])
def test_a_wrapped_base_is_destroyed_with_the_refined_index(pkg, data, kind):
    base = _trained(pkg, kind, data)
    cent = base.centroids()
    refined = pkg.refine_ann.FaissRefineFlat.wrap(base)
    assert refined.base is base and refined._owned and not base._owned
    base.close()  # a no-op: the handle went with the refined index
    assert base._h is not None and np.array_equal(base.centroids(), cent)
    with pytest.raises(ValueError, match="given its handle away"):
        pkg.refine_ann.FaissRefineFlat.wrap(base)
    with pytest.raises(ValueError, match="given its handle away"):
        pkg.polysemous_ann.adopt(base)
    refined.add(_rows(kind, data)[:N], data["ids"])
    ids, _, cnt = refined.search(_rows(kind, data)[:NQ], K, NPROBE)
    assert cnt.tolist() == [K] * NQ and np.isin(ids, data["ids"]).all(), "every cell is probed: k of the 64 rows come back"
    assert base.n == N
    refined.close()
    assert refined._h is None and base._h is None
    refined.close()
    base.close()
    assert refined._h is None and base._h is None
    with pytest.raises(pkg.ivf_ann.IvfError, match="null"):
        base.centroids()


@pytest.mark.parametrize("kind", ["pq", "opq"])
def test_an_adopted_index_answers_as_before(pkg, data, kind):
    ps = pkg.polysemous_ann
    ix = _trained(pkg, kind, data)
    ix.add(_rows(kind, data)[:N], data["ids"])
    q = _rows(kind, data)[:NQ]
    before = ps.search_ht(ix, q, K, NPROBE, 0)
    handle = ix._h
    twin = ps.adopt(ix)
    assert type(twin) is {"pq": ps.PolysemousIvfPq, "opq": ps.PolysemousOpqIvfPq}[kind] and ps.adopt(twin) is twin
    assert ix._h is None and not ix._owned and twin._h is handle and twin._owned
    ix.close()  # nothing to do: the twin holds the handle
    after = twin.search(q, K, NPROBE, ht=0)
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert before[2].tolist() == [K] * NQ
    with pytest.raises(ValueError, match="given its handle away"):
        ps.adopt(ix)
    twin.close()
    assert twin._h is None
    twin.close()


@pytest.mark.parametrize("kind", ["flat", "pq", "opq"])
def test_load_native_index_gives_back_the_saved_index(pkg, data, kind, tmp_path):
    ff = pkg.faiss_files
    saved = _trained(pkg, kind, data)
    saved.add(_rows(kind, data)[:N], data["ids"])
    ff.write_index(saved, tmp_path / kind)
    loaded = ff.load_native_index(D_IN if kind == "opq" else D, saved.metric, tmp_path / kind)
    assert type(loaded) is type(saved) and loaded._owned and loaded.FAISS_KIND == saved.FAISS_KIND == ff._kind_of(loaded)
    names = {"flat": ("metric", "d", "nlist"), "pq": ("metric", "d", "nlist", "M"), "opq": ("metric", "d", "d_in", "d_out", "nlist", "M")}
    for name in names[kind]:
        assert getattr(loaded, name) == getattr(saved, name), name
    assert loaded.metric is saved.metric and loaded.n == saved.n == N
    assert np.array_equal(loaded.centroids(), saved.centroids())
    saved.close()
    loaded.close()
    assert saved._h is None and loaded._h is None
