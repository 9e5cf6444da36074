"""The append entries of the ann JNI glue (AnnJni.hnswIndexAppend / denseIndexAppend) check every buffer's capacity and the
index handle before the library is called: a JVM caller gets a RuntimeException, never a read past a buffer."""
import ctypes as C

import numpy as np

import _jni
from _jni import ANN


def test_append_glue_checks_capacities(pkg):
    pkg.load_library()
    e = _jni.Env()
    x = np.zeros((4, 64), np.float32)
    for name, extra in (("hnswIndexAppend", (40, C.c_int64(1))), ("denseIndexAppend", ())):
        # vectors too small for n x d, ids too small for n, a negative n: refused before the (fake) index is touched
        _, msg, cls = e.call(ANN, name, None, C.c_int64(1), C.c_int64(5), 64, e.buffer(x), None, *extra)
        assert msg and "n x d floats" in msg and cls == "java/lang/RuntimeException", name
        _, msg, _ = e.call(ANN, name, None, C.c_int64(1), C.c_int64(4), 64, e.buffer(x), e.buffer(np.zeros(3, np.int64)), *extra)
        assert msg and "n x d floats" in msg, name
        _, msg, _ = e.call(ANN, name, None, C.c_int64(1), C.c_int64(-1), 64, e.buffer(x), None, *extra)
        assert msg and "n x d floats" in msg, name
        _, msg, _ = e.call(ANN, name, None, C.c_int64(1), C.c_int64(2), 64, None, None, *extra)
        assert msg and "n x d floats" in msg, name
        # a buffer whose capacity is short by one byte
        _, msg, _ = e.call(ANN, name, None, C.c_int64(1), C.c_int64(4), 64, e.buffer(x, 4 * 64 * 4 - 1), None, *extra)
        assert msg and "n x d floats" in msg, name
        # a null index
        _, msg, _ = e.call(ANN, name, None, C.c_int64(0), C.c_int64(4), 64, e.buffer(x), None, *extra)
        assert msg and "index" in msg, name
