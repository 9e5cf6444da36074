"""Build, append and search through the ann JNI glue (AnnJni.hnswIndexAppend / denseIndexAppend, executed with the hand-made
JNIEnv of tests/jni_harness.c) give what the Python path gives on the same calls."""
import ctypes as C

import numpy as np
import pytest

import _jni
from _jni import ANN

pytestmark = pytest.mark.gpu


def _search(e, fn, h, q, k, *ef):
    nq, d = q.shape
    dist, lab, cnt = np.zeros((nq, k), np.float32), np.zeros((nq, k), np.int64), np.zeros(nq, np.int32)
    _, msg, _ = e.call(ANN, fn, None, C.c_int64(h), nq, d, e.buffer(q), k, *ef, e.buffer(dist), e.buffer(lab), e.buffer(cnt))
    assert msg is None, msg
    return lab, dist, cnt


def _same(a, b):
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_append_through_the_glue_equals_the_python_path(pkg):
    e = _jni.Env()
    rng = np.random.default_rng(17)
    n0, n1, d = 3000, 1200, 64
    x = rng.standard_normal((n0 + n1, d)).astype(np.float32)
    keys = rng.permutation(10 * (n0 + n1))[:n0 + n1].astype(np.int64)
    q = rng.standard_normal((32, d)).astype(np.float32)
    m = pkg.dense_ann.DistanceMetric.L2

    # HNSW: the device builder (nThreads = 0), then appends
    h, msg, _ = e.call(ANN, "hnswIndexBuildInsert", C.c_int64, 0, int(m), C.c_int64(n0), d, e.buffer(x[:n0]), e.buffer(keys[:n0]), 8, 60,
                       C.c_int64(5), 0)
    assert msg is None and h
    py = pkg.hnsw_ann.Hnsw.build(m, x[:n0], ids=keys[:n0], max_m=8, ef_construction=60, seed=5, gpu=True)
    try:
        for a, b in ((n0, n0 + 700), (n0 + 700, n0 + n1)):
            _, msg, _ = e.call(ANN, "hnswIndexAppend", None, C.c_int64(h), C.c_int64(b - a), d, e.buffer(x[a:b]), e.buffer(keys[a:b]), 60,
                               C.c_int64(5))
            assert msg is None, msg
            py.append(x[a:b], keys[a:b], ef_construction=60, seed=5)
        _same(_search(e, "hnswSearch", h, q, 10, 50), py.search(q, 10, 50))
        # a duplicate key and a wrong dimension are RuntimeExceptions
        _, msg, cls = e.call(ANN, "hnswIndexAppend", None, C.c_int64(h), C.c_int64(1), d, e.buffer(x[:1]), e.buffer(keys[7:8]), 60, C.c_int64(5))
        assert msg and f"duplicate key {keys[7]}" in msg and cls == "java/lang/RuntimeException"
        _, msg, _ = e.call(ANN, "hnswIndexAppend", None, C.c_int64(h), C.c_int64(2), 32, e.buffer(x[:1]), e.buffer(keys[:2] + 10**9), 60, C.c_int64(5))
        assert msg and "dimension" in msg
        _same(_search(e, "hnswSearch", h, q, 10, 50), py.search(q, 10, 50))
    finally:
        py.close()
        e.call(ANN, "hnswIndexDestroy", None, C.c_int64(h))

    # brute force, fast and exact
    for exact in (0, 1):
        h, msg, _ = e.call(ANN, "denseIndexBuild", C.c_int64, 0, int(m), C.c_int64(n0), d, e.buffer(x[:n0]), e.buffer(keys[:n0]), C.c_uint8(exact))
        assert msg is None and h
        py = pkg.dense_ann.BruteForceIndex.build(m, x[:n0], keys[:n0], exact=bool(exact))
        try:
            _, msg, _ = e.call(ANN, "denseIndexAppend", None, C.c_int64(h), C.c_int64(n1), d, e.buffer(x[n0:]), e.buffer(keys[n0:]))
            assert msg is None, msg
            py.append(x[n0:], keys[n0:])
            _same(_search(e, "denseSearch", h, q, 20), py.search(q, 20))
            _, msg, _ = e.call(ANN, "denseIndexAppend", None, C.c_int64(h), C.c_int64(1), 32, e.buffer(x[:1]), e.buffer(keys[:1]))
            assert msg and "dimension" in msg
            _, msg, _ = e.call(ANN, "denseIndexAppend", None, C.c_int64(h), C.c_int64(1), d, e.buffer(x[:1]), None)
            assert msg and "ids" in msg
            _same(_search(e, "denseSearch", h, q, 20), py.search(q, 20))
        finally:
            py.close()
            e.call(ANN, "denseIndexDestroy", None, C.c_int64(h))
