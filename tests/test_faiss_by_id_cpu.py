"""include/faiss_by_id.h without a device: the exported symbols, the refusals that come before any device work, the Python
wrapper's shape / dtype checks and parameter refusals, and its distance translation over a stubbed library call."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1


@pytest.fixture(scope="module")
def fb(pkg):
    return importlib.import_module(pkg.__name__ + ".faiss_by_id")


@pytest.fixture(scope="module")
def sq(pkg):
    return importlib.import_module(pkg.__name__ + ".scalar_quantizer")


def test_library_exports_every_declared_symbol(pkg, fb):
    lib = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "faiss_by_id.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b([a-z_0-9]+)\s*\(", header))
    assert declared == {"ivf_by_id_last_error", "ivf_batch_query_by_id", "ivfsq_batch_query_by_id", "ivfpq_batch_query_by_id",
                        "opq_batch_query_by_id", "shard_set_batch_query_by_id", "ivf_by_id_last_stats"}
    assert declared == set(fb.PROTOS), "every declared symbol is bound and nothing else is"
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/faiss_by_id.h but not exported"


def test_package_does_not_reexport_the_subpackage(pkg, fb):
    assert not hasattr(pkg, "FaissQueryableById") and not hasattr(pkg, "FaissByIdError")
    assert issubclass(fb.FaissByIdError, pkg.ivf_ann.IvfError)


def test_arguments_are_refused_before_any_device_call(fb):
    lib = fb._lib()
    err = lambda: lib.ivf_by_id_last_error().decode()  # noqa: E731
    seeds = np.arange(4, dtype=np.int64)
    o_seed, o_id, o_dist, cnt = np.zeros(40, np.int64), np.zeros(40, np.int64), np.zeros(40, np.float32), np.zeros(4, np.int32)
    total = C.c_int64(-7)
    fake = C.c_void_p(1)  # never dereferenced: every call below is refused on its arguments

    for name, with_ht in (("ivf", False), ("ivfsq", False), ("ivfpq", True), ("opq", True), ("shard_set", True)):
        fn = getattr(lib, name + "_batch_query_by_id")

        def call(index=fake, store=fake, n=4, s=seeds, k=10, nprobe=4, cap=40, tot=C.byref(total), c=cnt, os_=o_seed, oi=o_id, od=o_dist):
            p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
            head = (index, store, n, p(s), k, nprobe) + ((0,) if with_ht else ())
            return fn(*head, p(os_), p(oi), p(od), cap, tot, p(c))

        assert call(index=None) == EINVAL and "NULL" in err(), name
        assert call(s=None) == EINVAL and "NULL" in err()
        assert call(tot=None) == EINVAL and "NULL" in err()
        assert call(c=None) == EINVAL and "NULL" in err()
        for kw in ("os_", "oi", "od"):
            assert call(**{kw: None}) == EINVAL and "NULL" in err(), (name, kw)
        for k in (0, -1, 1025):
            assert call(k=k) == EINVAL and "k must be in 1..1024" in err()
        for nprobe in (0, -1, 1025):
            assert call(nprobe=nprobe) == EINVAL and "nprobe must be in 1..1024" in err()
        assert call(n=-1) == EINVAL and "n_seeds" in err()
        assert call(n=0x7fffffff) == EINVAL and "n_seeds" in err()
        assert call(cap=-1) == EINVAL and "cap" in err()
        assert call(store=None) == EINVAL and "store" in err() and "no fp32 rows of its own" in err()
    assert total.value == -7 and not o_seed.any() and not o_id.any() and not o_dist.any() and not cnt.any()  # nothing was written
    assert lib.ivf_by_id_last_stats(1, None, *([None] * 8)) == EINVAL and "NULL" in err()
    assert lib.ivf_by_id_last_stats(0, fake, *([None] * 8)) == EINVAL and "kind_or_set" in err()
    assert lib.ivf_by_id_last_stats(6, fake, *([None] * 8)) == EINVAL and "kind_or_set" in err()


def _stub_indexes(pkg, sq):
    """Index objects that own nothing: every check below comes before any native call."""
    M = pkg.dense_ann.DistanceMetric
    return {"flat": pkg.ivf_ann.FaissIvfFlat(None, M.L2, 32, 8), "sq8": sq.FaissIvfSq8(None, M.L2, 32, 8),
            "pq": pkg.ivfpq_ann.FaissIvfPq(None, M.L2, 32, 8, 8), "opq": pkg.opq_ann.FaissOpqIvfPq(None, M.L2, 40, 32, 8, 8),
            "set": pkg.shard_set.ShardSet(None, M.L2, 32, 0)}


def test_python_wrapper_checks_shapes_dtypes_and_parameters(pkg, fb, sq):
    M, P = pkg.dense_ann.DistanceMetric, pkg.ivf_ann.FaissParams
    ix = _stub_indexes(pkg, sq)
    st32, st40 = pkg.ann_by_id.EmbeddingStore(None, 5, 32), pkg.ann_by_id.EmbeddingStore(None, 5, 40)
    with pytest.raises(TypeError, match="EmbeddingStore"):
        fb.FaissQueryableById(None, ix["flat"], M.L2)
    with pytest.raises(TypeError, match="index must be"):
        fb.FaissQueryableById(st32, pkg.dense_ann.BruteForceIndex(None, 0, 10, 32), M.L2)
    with pytest.raises(ValueError, match="dimension"):
        fb.FaissQueryableById(st40, ix["flat"], M.L2)
    with pytest.raises(ValueError, match="d_in"):
        fb.FaissQueryableById(st32, ix["opq"], M.L2)  # the store holds d_in-wide rows
    fb.FaissQueryableById(st40, ix["opq"], M.L2)
    q = fb.FaissQueryableById(st32, ix["flat"], M.L2)
    with pytest.raises(TypeError, match="FaissParams"):
        q.batchQueryById([1, 2], 10, None)
    with pytest.raises(ValueError, match="nprobe must be set"):
        q.batchQueryById([1, 2], 10, P())
    with pytest.raises(ValueError, match="positive"):
        q.batchQueryById([1, 2], 0, P(nprobe=4))
    with pytest.raises(ValueError, match="one-dimensional"):
        q.batchQueryById([[1, 2]], 10, P(nprobe=4))
    with pytest.raises(ValueError, match="integers"):
        q.queryById(1.5, 10, P(nprobe=4))
    for field in ("quantizerKfactorRf", "quantizerNprobe"):
        for name in ix:
            store = st40 if name == "opq" else st32
            with pytest.raises(ValueError, match=field):
                fb.FaissQueryableById(store, ix[name], M.L2).batchQueryById([1], 10, P(nprobe=4, **{field: 2}))
    for name in ("flat", "sq8"):  # ht is refused by name where the index has no codes ...
        with pytest.raises(ValueError, match="ht cannot be set"):
            fb.FaissQueryableById(st32, ix[name], M.L2).batchQueryById([1], 10, P(nprobe=4, ht=20))
    for name in ("sq8", "set"):  # ... and quantizerEf where it carries no graph
        with pytest.raises(ValueError, match="quantizerEf cannot be set"):
            fb.FaissQueryableById(st32, ix[name], M.L2).batchQueryById([1], 10, P(nprobe=4, quantizerEf=8))


def test_translation_is_faiss_queryables_over_a_stubbed_call(pkg, fb, sq, monkeypatch):
    """What the wrapper returns is what FaissQueryable.queryWithDistance returns for the same rows, the Cosine clamp included."""
    M, P = pkg.dense_ann.DistanceMetric, pkg.ivf_ann.FaissParams
    # three seeds: two rows of different lengths around an absent seed; Cosine distances on both sides of the clamp
    rows = {7: (np.array([70, 71, 72], np.int64), np.array([-0.25, 0.5, 1.75], np.float32)),
            9: (np.array([90], np.int64), np.array([2.5], np.float32))}
    seeds = [7, 8, 9]

    class StubIndex:
        def __init__(self, row):
            self.row = row

        def search(self, queries, k, nprobe):
            ids, dist = self.row
            out_i, out_d = np.zeros((1, k), np.int64), np.zeros((1, k), np.float32)
            out_i[0, :len(ids)], out_d[0, :len(ids)] = ids, dist
            return out_i, out_d, np.array([len(ids)], np.int32)

    for metric in (M.Cosine, M.L2, M.InnerProduct):
        q = fb.FaissQueryableById(pkg.ann_by_id.EmbeddingStore(None, 5, 32), _stub_indexes(pkg, sq)["flat"], metric)

        def batch_arrays(ids, k, params, cap=None):
            assert params.nprobe == 4
            s = np.concatenate([np.full(len(rows[i][0]), i, np.int64) for i in ids if i in rows] or [np.zeros(0, np.int64)])
            i_ = np.concatenate([rows[i][0] for i in ids if i in rows] or [np.zeros(0, np.int64)])
            d_ = np.concatenate([rows[i][1] for i in ids if i in rows] or [np.zeros(0, np.float32)])
            return s, i_, d_, np.array([len(rows[i][0]) if i in rows else -1 for i in ids], np.int32)

        monkeypatch.setattr(q, "batch_arrays", batch_arrays)
        want = []
        for s in seeds:
            if s in rows:
                want += [(s, i, d) for i, d in pkg.ivf_ann.FaissQueryable(StubIndex(rows[s]), metric).queryWithDistance(np.zeros(32), 10, P(nprobe=4))]
        got = q.batchQueryWithDistanceById(seeds, 10, P(nprobe=4))
        assert got == want and len(got) == 4
        if metric == M.Cosine:  # similarity 1.25 and -0.75, -1.5 are outside [0, 1]: MAX_COSINE_DISTANCE
            assert [d for _, _, d in got] == [1.0, 0.5, 1.0, 1.0]
        else:
            assert [d for _, _, d in got] == [-0.25, 0.5, 1.75, 2.5]
        assert q.batchQueryById(seeds, 10, P(nprobe=4)) == [(s, i) for s, i, _ in want]
        assert q.queryByIdWithDistance(7, 10, P(nprobe=4)) == [(i, d) for s, i, d in want if s == 7]
        assert q.queryById(8, 10, P(nprobe=4)) == []
        assert q.queryById(9, 10, P(nprobe=4)) == [90]
