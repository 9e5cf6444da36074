"""Builds tests/hnsw_update_ref.c (the CPU restatement of hnsw_index_update) with gcc and wraps it."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_state = {}


def load():
    if "lib" in _state:
        return _state["lib"]
    d = tempfile.mkdtemp(prefix="hnswupd_")
    out = os.path.join(d, "libhnsw_update_ref.so")
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra",
                    "-Wno-unused-parameter", "-Wno-unused-function", os.path.join(ROOT, "tests", "hnsw_update_ref.c"), "-o", out, "-lm"],
                   check=True)
    lib = C.CDLL(out)
    lib.ref_hnsw_update.restype = C.c_int64
    _state["lib"] = lib
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def update(metric, stored, graph, max_m, ef_construction, rows, pos, batch, ccap=1024, link_cap=1024):
    """The graph after hnsw_index_update of `rows` (stored form: fp16-rounded, normalised for Cosine) at positions `pos`, from
    `graph` over `stored` (the rows before).  batch = 0: HnswIndex.reInsert once per row.  Returns (graph, stats) with stats =
    (rounds, relinks, superseded, additions already present, lists kept); graph entries sorted by (level, item)."""
    L = load()
    x = np.ascontiguousarray(stored, np.float32)
    r = np.ascontiguousarray(rows, np.float32).reshape(-1, x.shape[1])
    ps = np.ascontiguousarray(pos, np.int64)
    lv, it, off, nb, entry, max_level = graph
    lv = np.ascontiguousarray(lv, np.int32); it = np.ascontiguousarray(it, np.int64)
    off = np.ascontiguousarray(off, np.int64); nb = np.ascontiguousarray(nb, np.int64)
    if nb.size == 0:
        nb = np.zeros(1, np.int64)
    n = x.shape[0]
    top = max(int(max_level), int(lv.max()) if lv.size else 0)
    cap_e = n * (top + 1) + 1
    cap_n = cap_e * 2 * max_m
    o_lv = np.zeros(cap_e, np.int32); o_it = np.zeros(cap_e, np.int64); o_off = np.zeros(cap_e + 1, np.int64)
    o_nb = np.zeros(cap_n, np.int64)
    o_entry = C.c_int64(); o_ml = C.c_int32()
    stats = np.zeros(5, np.int64)
    ne = L.ref_hnsw_update(C.c_int32(int(metric)), C.c_int64(n), C.c_int32(x.shape[1]), _p(x), C.c_int32(max_m), C.c_int32(ef_construction),
                           C.c_int64(int(entry)), C.c_int32(int(max_level)), C.c_int64(len(lv)), _p(lv), _p(it), _p(off), _p(nb),
                           C.c_int64(len(ps)), _p(r), _p(ps), C.c_int32(batch), C.c_int32(ccap), C.c_int32(link_cap), C.c_int64(cap_e),
                           C.c_int64(cap_n), _p(o_lv), _p(o_it), _p(o_off), _p(o_nb), C.byref(o_entry), C.byref(o_ml), _p(stats))
    assert ne >= 0
    return (o_lv[:ne], o_it[:ne], o_off[:ne + 1], o_nb[:o_off[ne]], o_entry.value, o_ml.value), tuple(int(s) for s in stats)


def as_dict(graph):
    """{(level, item): [neighbours]} of a flat graph, for comparisons independent of entry order."""
    lv, it, off, nb = graph[:4]
    return {(int(lv[e]), int(it[e])): [int(v) for v in nb[off[e]:off[e + 1]]] for e in range(len(lv))}
