"""ctypes binding of include/ivf_ann.h and a host-side mirror of the reference's Faiss queryable.

Reference (paths relative to the reference's ann/src/main/):
  scala/com/twitter/ann/faiss/FaissIndexer.scala:82-92            index_factory -> train -> add_with_ids
  scala/com/twitter/ann/faiss/QueryableIndexAdapter.scala:139-178 queryWithDistance
  scala/com/twitter/ann/faiss/QueryableIndexAdapter.scala:52-65   maybeTranslateToCosineDistanceInplace
  scala/com/twitter/ann/faiss/FaissCommon.scala:11-37             FaissParams <-> FaissRuntimeParam
  thrift/com/twitter/ann/common/ann_common.thrift:41-56           FaissRuntimeParam
Only `IVF<nlist>,Flat` exists on the device: of the runtime parameters only nprobe means anything to it.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .dense_ann import DistanceMetric
from .simclusters_ann import load_library

_P = C.POINTER
PROTOS = {
    "ivf_last_error": (C.c_char_p, []),
    "ivf_index_train": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_uint64,
                                  _P(C.c_void_p)]),
    "ivf_index_load": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, _P(C.c_void_p)]),
    "ivf_index_add": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ivf_search": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ivf_index_info": (C.c_int, [C.c_void_p, _P(C.c_int64), _P(C.c_int32), _P(C.c_int32), _P(C.c_int32)]),
    "ivf_index_get_centroids": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ivf_index_list_sizes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ivf_index_get_assignment": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ivf_last_probes": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), C.c_void_p]),
    "ivf_last_stats": (C.c_int, [C.c_void_p, _P(C.c_int64), _P(C.c_int32), _P(C.c_float), _P(C.c_float), _P(C.c_float)]),
    "ivf_index_destroy": (C.c_int, [C.c_void_p]),
}

MAX_COSINE_DISTANCE = 1.0


class IvfError(RuntimeError):
    pass


def _lib():
    lib = load_library()
    if not getattr(lib, "_ivf_ready", False):
        for name, (res, args) in PROTOS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        lib._ivf_ready = True
    return lib


def _check(lib, rc: int) -> None:
    if rc != 0:
        raise IvfError(f"ivf_ann error {rc}: {lib.ivf_last_error().decode()}")


def _rows(a, d: Optional[int] = None) -> np.ndarray:
    v = np.ascontiguousarray(a, np.float32)
    if v.ndim == 1:
        v = v[None, :]
    if v.ndim != 2 or (d is not None and v.shape[1] != d):
        raise ValueError(f"expected rows of dimension {d}, got shape {v.shape}")
    return v


class FaissIvfFlat:
    """`IVF<nlist>,Flat` in an id map, resident in HBM: train() or load() the coarse quantizer, add() rows, search()."""

    def __init__(self, handle, metric: DistanceMetric, d: int, nlist: int):
        self._h, self.metric, self.d, self.nlist = handle, DistanceMetric(metric), d, nlist

    @classmethod
    def train(cls, metric: DistanceMetric, nlist: int, train_vectors: np.ndarray, *, niter: int = 0, seed: int = 1, device: int = 0):
        """Deterministic Lloyd's k-means over train_vectors (niter: 0 = 20 rounds, -1 = the initial picks)."""
        lib = _lib()
        v = _rows(train_vectors)
        h = C.c_void_p()
        _check(lib, lib.ivf_index_train(device, int(metric), v.shape[1], nlist, v.shape[0], v.ctypes.data, niter, seed, C.byref(h)))
        return cls(h, metric, v.shape[1], nlist)

    @classmethod
    def load(cls, metric: DistanceMetric, centroids: np.ndarray, *, device: int = 0):
        lib = _lib()
        c = _rows(centroids)
        h = C.c_void_p()
        _check(lib, lib.ivf_index_load(device, int(metric), c.shape[1], c.shape[0], c.ctypes.data, C.byref(h)))
        return cls(h, metric, c.shape[1], c.shape[0])

    @property
    def n(self) -> int:
        n = C.c_int64()
        lib = _lib()
        _check(lib, lib.ivf_index_info(self._h, C.byref(n), None, None, None))
        return n.value

    def add(self, vectors: np.ndarray, ids: Optional[Sequence[int]] = None) -> None:
        """add_with_ids.  ids on every call or on none (ids = positions in the order added)."""
        lib = _lib()
        v = _rows(vectors, self.d)
        idp = None
        if ids is not None:
            idp = np.ascontiguousarray(ids, np.int64)
            if idp.shape != (v.shape[0],):
                raise ValueError("one id per vector")
        _check(lib, lib.ivf_index_add(self._h, v.shape[0], v.ctypes.data, idp.ctypes.data if idp is not None else None))

    def search(self, queries: np.ndarray, k: int, nprobe: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(ids [nq, k], distances [nq, k], counts [nq]): the k nearest rows of the nprobe nearest cells' lists, ascending
        by (distance, id); counts may fall short of k."""
        lib = _lib()
        q = _rows(queries, self.d)
        nq = q.shape[0]
        dist = np.zeros((nq, k), np.float32)
        ids = np.zeros((nq, k), np.int64)
        cnt = np.zeros(nq, np.int32)
        _check(lib, lib.ivf_search(self._h, nq, q.ctypes.data, k, nprobe, dist.ctypes.data, ids.ctypes.data, cnt.ctypes.data))
        return ids, dist, cnt

    def centroids(self) -> np.ndarray:
        out = np.empty((self.nlist, self.d), np.float32)
        lib = _lib()
        _check(lib, lib.ivf_index_get_centroids(self._h, out.ctypes.data))
        return out

    def list_sizes(self) -> np.ndarray:
        out = np.empty(self.nlist, np.int64)
        lib = _lib()
        _check(lib, lib.ivf_index_list_sizes(self._h, out.ctypes.data))
        return out

    def assignment(self) -> Tuple[np.ndarray, np.ndarray]:
        """(ids [n], cells [n]) of the rows in the order they were added."""
        n = self.n
        ids, cells = np.empty(n, np.int64), np.empty(n, np.int32)
        lib = _lib()
        _check(lib, lib.ivf_index_get_assignment(self._h, ids.ctypes.data, cells.ctypes.data))
        return ids, cells

    def last_probes(self) -> np.ndarray:
        """The cells the last search probed, nearest first: int32 [nq, nprobe] (nprobe after clamping to nlist)."""
        nq, npr = C.c_int32(), C.c_int32()
        lib = _lib()
        _check(lib, lib.ivf_last_probes(self._h, C.byref(nq), C.byref(npr), None))
        out = np.empty((nq.value, npr.value), np.int32)
        _check(lib, lib.ivf_last_probes(self._h, None, None, out.ctypes.data))
        return out

    def last_stats(self) -> dict:
        rows, rounds = C.c_int64(), C.c_int32()
        a, b, s = C.c_float(), C.c_float(), C.c_float()
        lib = _lib()
        _check(lib, lib.ivf_last_stats(self._h, C.byref(rows), C.byref(rounds), C.byref(a), C.byref(b), C.byref(s)))
        return {"rows_scanned": rows.value, "rounds": rounds.value, "coarse_ms": a.value, "scan_ms": b.value, "select_ms": s.value}

    def close(self) -> None:
        if self._h:
            _lib().ivf_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass(frozen=True)
class FaissParams:
    """FaissRuntimeParam (ann_common.thrift:41-56), every field optional as there."""

    nprobe: Optional[int] = None
    quantizerEf: Optional[int] = None
    quantizerKfactorRf: Optional[int] = None
    quantizerNprobe: Optional[int] = None
    ht: Optional[int] = None


class FaissQueryable:
    """QueryableIndexAdapter.queryWithDistance (:139-178) on top of FaissIvfFlat.search.  The index answers distances
    already (1 - similarity for Cosine); the adapter's Cosine translation (:52-65) is reproduced on the similarity they
    stand for: one outside [0, 1] becomes MAX_COSINE_DISTANCE, the order stays as returned."""

    def __init__(self, index, metric: DistanceMetric):
        self.index, self.metric = index, DistanceMetric(metric)

    @staticmethod
    def _nprobe(params: FaissParams) -> int:
        others = [f for f in ("quantizerEf", "quantizerKfactorRf", "quantizerNprobe", "ht") if getattr(params, f) is not None]
        if others:
            raise ValueError("an IVF-Flat index has no HNSW quantizer, refinement or polysemous codes: "
                             + ", ".join(others) + " cannot be set (only nprobe)")
        if params.nprobe is None:
            raise ValueError("FaissParams.nprobe must be set")
        return int(params.nprobe)

    def queryWithDistance(self, embedding: np.ndarray, numOfNeighbors: int, runtimeParams: FaissParams) -> List[Tuple[int, float]]:
        nprobe = self._nprobe(runtimeParams)
        ids, dist, cnt = self.index.search(np.asarray(embedding, np.float32), numOfNeighbors, nprobe)
        m = int(cnt[0])
        out_d = np.array(dist[0, :m], np.float32)
        if self.metric == DistanceMetric.Cosine:
            sim = np.float32(1.0) - out_d
            out_d = np.where((sim < 0) | (sim > 1), np.float32(MAX_COSINE_DISTANCE), out_d).astype(np.float32)
        return list(zip(np.asarray(ids[0, :m]).tolist(), out_d.tolist()))

    def query(self, embedding: np.ndarray, numOfNeighbors: int, runtimeParams: FaissParams) -> List[int]:
        return [i for i, _ in self.queryWithDistance(embedding, numOfNeighbors, runtimeParams)]
