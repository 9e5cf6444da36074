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

from . import binding as _binding
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
# FAISS_KIND_* of include/faiss_files.h
KIND_IVF_FLAT, KIND_IVF_PQ, KIND_OPQ_IVF_PQ = 1, 2, 3


class IvfError(RuntimeError):
    pass


_lib = _binding.binder(PROTOS, "ivf", load_library)
_check = _binding.checker(IvfError, "ivf_ann", "ivf_last_error")
_rows = _binding.rows


class _IvfFamilyIndex(_binding.Handle):
    """What FaissIvfFlat, FaissIvfPq and FaissOpqIvfPq share: the calls whose C symbols differ by their prefix alone.  A
    subclass names its prefix, its module's _lib / _check, the attribute that holds the dimension of incoming rows, its
    FAISS_KIND_* of include/faiss_files.h and how many int32 fields its *_index_info reports after n."""

    _prefix = ""
    _check = None
    _row_dim = "d"
    _info_fields = 0
    _STATS = ("coarse_ms", "scan_ms", "select_ms")  # the float fields of *_last_stats
    FAISS_KIND = 0

    def _call(self, name: str, *args) -> None:
        lib = self._lib()
        self._check(lib, getattr(lib, self._prefix + name)(self._h, *args))

    @classmethod
    def _read_info(cls, handle):
        """(n, the int32 fields) of *_index_info."""
        n, v = C.c_int64(), [C.c_int32() for _ in range(cls._info_fields)]
        lib = cls._lib()
        cls._check(lib, getattr(lib, cls._prefix + "_index_info")(handle, C.byref(n), *[C.byref(x) for x in v]))
        return n.value, [x.value for x in v]

    @property
    def n(self) -> int:
        return self._read_info(self._h)[0]

    def add(self, vectors: np.ndarray, ids: Optional[Sequence[int]] = None) -> None:
        """add_with_ids.  ids on every call or on none (ids = positions in the order added)."""
        v = _rows(vectors, getattr(self, self._row_dim))
        idp = _binding.ids_or_none(ids, v.shape[0])
        self._call("_index_add", v.shape[0], v.ctypes.data, _binding.ptr(idp))

    def search(self, queries: np.ndarray, k: int, nprobe: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(ids [nq, k], distances [nq, k], counts [nq]): the k nearest rows (IVF-Flat) or codes (IVF-PQ; OPQ: over the
        transformed queries) of the nprobe nearest cells' lists, ascending by (distance, id); counts may fall short of k."""
        q = _rows(queries, getattr(self, self._row_dim))
        ids, dist, cnt = _binding.result_triple(q.shape[0], k)
        self._call("_search", q.shape[0], q.ctypes.data, k, nprobe, dist.ctypes.data, ids.ctypes.data, cnt.ctypes.data)
        return ids, dist, cnt

    def centroids(self) -> np.ndarray:
        out = np.empty((self.nlist, self.d), np.float32)
        self._call("_index_get_centroids", out.ctypes.data)
        return out

    def list_sizes(self) -> np.ndarray:
        out = np.empty(self.nlist, np.int64)
        self._call("_index_list_sizes", out.ctypes.data)
        return out

    def assignment(self) -> Tuple[np.ndarray, np.ndarray]:
        """(ids [n], cells [n]) of the rows in the order they were added."""
        n = self.n
        ids, cells = np.empty(n, np.int64), np.empty(n, np.int32)
        self._call("_index_get_assignment", ids.ctypes.data, cells.ctypes.data)
        return ids, cells

    def last_probes(self) -> np.ndarray:
        """The cells the last search probed, nearest first: int32 [nq, nprobe] (nprobe after clamping to nlist)."""
        nq, npr = C.c_int32(), C.c_int32()
        self._call("_last_probes", C.byref(nq), C.byref(npr), None)
        out = np.empty((nq.value, npr.value), np.int32)
        self._call("_last_probes", None, None, out.ctypes.data)
        return out

    def last_stats(self) -> dict:
        rows, rounds = C.c_int64(), C.c_int32()
        ms = [C.c_float() for _ in self._STATS]
        self._call("_last_stats", C.byref(rows), C.byref(rounds), *[C.byref(x) for x in ms])
        return {"rows_scanned": rows.value, "rounds": rounds.value, **{name: x.value for name, x in zip(self._STATS, ms)}}


class FaissIvfFlat(_IvfFamilyIndex):
    """`IVF<nlist>,Flat` in an id map, resident in HBM: train() or load() the coarse quantizer, add() rows, search()."""

    _prefix, _destroy, _info_fields, FAISS_KIND = "ivf", "ivf_index_destroy", 3, KIND_IVF_FLAT
    _lib, _check = staticmethod(_lib), staticmethod(_check)

    def __init__(self, handle, metric: DistanceMetric, d: int, nlist: int):
        self._h, self.metric, self.d, self.nlist = handle, DistanceMetric(metric), d, nlist

    @classmethod
    def _from_handle(cls, handle):
        _, (d, metric, nlist) = cls._read_info(handle)
        return cls(handle, DistanceMetric(metric), d, nlist)

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
