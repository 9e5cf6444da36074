"""include/ann_by_id.h without a device: the exported symbols, the refusals that come before any device work, the Python wrappers'
shape / dtype checks and the JNI glue's capacity checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _jni
from _jni import ANN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(pkg):
    lib = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "ann_by_id.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    names = set(re.findall(r"\b((?:ann_store|ann_by_id|hnsw_batch|dann_batch)\w*)\s*\(", header))
    assert {"ann_store_build", "ann_store_info", "ann_store_get", "ann_store_destroy", "ann_by_id_last_error", "ann_by_id_last_stats",
            "hnsw_batch_query_by_id", "dann_batch_query_by_id"} <= names
    for name in names:
        assert hasattr(lib, name), f"{name} declared in include/ann_by_id.h but not exported"
    for name in pkg.ann_by_id.PROTOS:
        assert name in names, f"{name} bound by ann_by_id.py but not declared in the header"


def test_arguments_are_refused_before_any_device_call(pkg):
    b = pkg.ann_by_id
    lib = b._lib()
    err = lambda: lib.ann_by_id_last_error().decode()  # noqa: E731
    seeds = np.arange(4, dtype=np.int64)
    o_seed, o_id, o_dist, cnt = np.zeros(40, np.int64), np.zeros(40, np.int64), np.zeros(40, np.float32), np.zeros(4, np.int32)
    total = C.c_int64(-7)
    fake = C.c_void_p(1)  # never dereferenced: every call below is refused on its arguments

    def hnsw(index=None, n=4, s=seeds, k=10, ef=50, cap=40, tot=C.byref(total), c=cnt, os_=o_seed):
        return lib.hnsw_batch_query_by_id(index, None, n, None if s is None else s.ctypes.data, k, ef, None if os_ is None else os_.ctypes.data,
                                          o_id.ctypes.data, o_dist.ctypes.data, cap, tot, None if c is None else c.ctypes.data)

    def dann(index=None, n=4, s=seeds, k=10, cap=40, tot=C.byref(total), c=cnt):
        return lib.dann_batch_query_by_id(index, None, n, None if s is None else s.ctypes.data, k, o_seed.ctypes.data, o_id.ctypes.data,
                                          o_dist.ctypes.data, cap, tot, None if c is None else c.ctypes.data)

    assert hnsw() == 1 and "NULL" in err()                       # NULL index
    assert dann() == 1 and "NULL" in err()
    assert hnsw(index=fake, s=None) == 1 and "NULL" in err()     # NULL seeds
    assert hnsw(index=fake, tot=None) == 1 and "NULL" in err()   # NULL out_total
    assert hnsw(index=fake, c=None) == 1 and "NULL" in err()     # NULL out_counts
    assert hnsw(index=fake, os_=None) == 1 and "NULL" in err()   # NULL out_seed with cap > 0
    assert dann(index=fake, s=None) == 1 and "NULL" in err()
    assert hnsw(k=0) == 1 and "positive" in err()                # k < 1, the plain search's code and words
    assert hnsw(ef=0) == 1 and "positive" in err()
    assert dann(k=0) == 1 and "1..1024" in err()
    assert dann(k=1025) == 1 and "1..1024" in err()
    assert hnsw(index=fake, cap=-1) == 1 and "cap" in err()      # a cap that can hold nothing
    assert dann(index=fake, cap=-1) == 1 and "cap" in err()
    assert hnsw(index=fake, n=-1) == 1 and "n_seeds" in err()
    assert total.value == -7 and not o_seed.any() and not cnt.any()  # nothing was written
    # the store
    h = C.c_void_p()
    v = np.zeros((4, 8), np.float32)
    assert lib.ann_store_build(0, 4, 8, seeds.ctypes.data, v.ctypes.data, None) == 1 and "NULL" in err()
    assert lib.ann_store_build(0, 4, 0, seeds.ctypes.data, v.ctypes.data, C.byref(h)) == 1 and "1..512" in err()
    assert lib.ann_store_build(0, 4, 513, seeds.ctypes.data, v.ctypes.data, C.byref(h)) == 1 and "1..512" in err()
    assert lib.ann_store_build(0, -1, 8, seeds.ctypes.data, v.ctypes.data, C.byref(h)) == 1 and "row count" in err()
    assert lib.ann_store_build(0, 4, 8, None, v.ctypes.data, C.byref(h)) == 1 and "NULL" in err()
    assert lib.ann_store_build(0, 4, 8, seeds.ctypes.data, None, C.byref(h)) == 1 and "NULL" in err()
    assert not h.value
    assert lib.ann_store_info(None, None, None) == 1 and "NULL" in err()
    assert lib.ann_store_get(None, 1, seeds.ctypes.data, v.ctypes.data, cnt.ctypes.data) == 1 and "NULL" in err()
    assert lib.ann_store_destroy(None) == 0
    assert lib.ann_by_id_last_stats(None, None, *([None] * 8)) == 1 and "exactly one" in err()
    assert lib.ann_by_id_last_stats(fake, fake, *([None] * 8)) == 1 and "exactly one" in err()


def test_python_wrappers_check_shapes_and_dtypes(pkg):
    b = pkg.ann_by_id
    with pytest.raises(ValueError, match="one-dimensional"):
        b.EmbeddingStore.build(np.zeros((2, 2), np.int64), np.zeros((2, 4), np.float32))
    with pytest.raises(ValueError, match="integers"):
        b.EmbeddingStore.build(np.zeros(2, np.float32), np.zeros((2, 4), np.float32))
    with pytest.raises(ValueError, match=r"\[n\]\[d\]"):
        b.EmbeddingStore.build(np.zeros(2, np.int64), np.zeros(8, np.float32))
    with pytest.raises(ValueError, match="floating"):
        b.EmbeddingStore.build(np.zeros(2, np.int64), np.zeros((2, 4), np.int32))
    with pytest.raises(ValueError, match="one key per vector"):
        b.EmbeddingStore.build(np.zeros(3, np.int64), np.zeros((2, 4), np.float32))
    with pytest.raises(TypeError, match="Hnsw or a BruteForceIndex"):
        b.QueryableById(None, object())
    hn = pkg.hnsw_ann.Hnsw(None, 0, 10, 16, 8)          # handles that own nothing: the checks below come before any call
    bf = pkg.dense_ann.BruteForceIndex(None, 0, 10, 16)
    st = b.EmbeddingStore(None, 5, 32)
    with pytest.raises(TypeError, match="EmbeddingStore or None"):
        b.QueryableById(object(), hn)
    with pytest.raises(ValueError, match="dimension"):
        b.QueryableById(st, hn)
    with pytest.raises(ValueError, match="dimension"):
        b.QueryableById(st, bf)
    q = b.QueryableById(None, hn)
    with pytest.raises(TypeError, match="HnswParams"):
        q.batchQueryWithDistanceById([1, 2], 10)
    with pytest.raises(ValueError, match="positive"):
        q.batchQueryById([1, 2], 0, pkg.hnsw_ann.HnswParams(50))
    with pytest.raises(ValueError, match="one-dimensional"):
        q.batchQueryById([[1, 2]], 10, pkg.hnsw_ann.HnswParams(50))
    with pytest.raises(ValueError, match="integers"):
        b.QueryableById(None, bf).batchQueryById([1.5], 10)
    assert pkg.QueryableById is b.QueryableById and pkg.EmbeddingStore is b.EmbeddingStore


def test_jni_glue_checks_capacities_before_any_native_call():
    e = _jni.Env()
    keys, vec = np.zeros(4, np.int64), np.zeros((4, 8), np.float32)
    r, msg, cls = e.call(ANN, "embeddingStoreBuild", C.c_int64, 0, C.c_int64(5), 8, e.buffer(keys), e.buffer(np.zeros((5, 8), np.float32)))
    assert r == 0 and "n longs" in msg and cls == "java/lang/RuntimeException"
    r, msg, _ = e.call(ANN, "embeddingStoreBuild", C.c_int64, 0, C.c_int64(5), 8, e.buffer(np.zeros(5, np.int64)), e.buffer(vec))
    assert r == 0 and "n x d floats" in msg
    r, msg, _ = e.call(ANN, "embeddingStoreBuild", C.c_int64, 0, C.c_int64(4), 8, None, e.buffer(vec))
    assert r == 0 and msg
    r, msg, _ = e.call(ANN, "embeddingStoreBuild", C.c_int64, 0, C.c_int64(-1), 8, e.buffer(keys), e.buffer(vec))
    assert r == 0 and msg
    seeds = np.zeros(4, np.int64)

    def bufs(n_seed=4, n_oseed=40, n_oid=40, n_odist=40, n_cnt=4):
        return (e.buffer(np.zeros(n_seed, np.int64)), e.buffer(np.zeros(n_oseed, np.int64)), e.buffer(np.zeros(n_oid, np.int64)),
                e.buffer(np.zeros(n_odist, np.float32)), e.buffer(np.zeros(n_cnt, np.int32)))

    for name, extra in (("hnswBatchQueryById", (50,)), ("denseBatchQueryById", ())):
        def call(index=1, n=4, k=10, cap=40, **kw):
            s, os_, oi, od, oc = bufs(**kw)
            return e.call(ANN, name, C.c_int64, C.c_int64(index), C.c_int64(0), n, s, k, *extra, os_, oi, od, C.c_int64(cap), oc)

        for kw in (dict(n_seed=3), dict(n_oseed=39), dict(n_oid=39), dict(n_odist=39), dict(n_cnt=3)):
            r, msg, _ = call(**kw)
            assert r == 0 and "smaller than" in msg, (name, kw)
        r, msg, _ = call(index=0)
        assert r == 0 and "index" in msg
        r, msg, _ = call(k=0)
        assert r == 0 and "k >= 1" in msg
        r, msg, _ = call(cap=-1)
        assert r == 0 and "cap >= 0" in msg
    del seeds
