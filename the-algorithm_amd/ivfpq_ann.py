"""ctypes binding of include/ivfpq_ann.h (`IVF<nlist>,PQ<M>`), Faiss's index_factory for the strings the device can serve,
and the reference's index build.

Reference (paths relative to the reference's ann/src/main/):
  scala/com/twitter/ann/faiss/FaissIndexer.scala:82-92            index_factory -> train -> add_with_ids
  thrift/com/twitter/ann/common/ann_common.thrift:45              nprobe: "How many cells to visit in IVFPQ"
FaissQueryable (ivf_ann.py) works over FaissIvfPq unchanged: it needs search() alone.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import Optional, Sequence, Tuple

import numpy as np

from .dense_ann import DistanceMetric
from .ivf_ann import FaissIvfFlat, IvfError, _rows
from .simclusters_ann import load_library

_P = C.POINTER
PROTOS = {
    "ivfpq_last_error": (C.c_char_p, []),
    "ivfpq_index_train": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int32,
                                    C.c_uint64, _P(C.c_void_p)]),
    "ivfpq_index_load": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, _P(C.c_void_p)]),
    "ivfpq_index_add": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ivfpq_search": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ivfpq_index_info": (C.c_int, [C.c_void_p, _P(C.c_int64), _P(C.c_int32), _P(C.c_int32), _P(C.c_int32), _P(C.c_int32)]),
    "ivfpq_index_get_centroids": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ivfpq_index_get_codebooks": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ivfpq_index_get_codes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ivfpq_index_list_sizes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ivfpq_index_get_assignment": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ivfpq_last_probes": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), C.c_void_p]),
    "ivfpq_last_stats": (C.c_int, [C.c_void_p, _P(C.c_int64), _P(C.c_int32), _P(C.c_float), _P(C.c_float), _P(C.c_float)]),
    "ivfpq_index_destroy": (C.c_int, [C.c_void_p]),
}

KSUB = 256  # codewords per sub-quantizer (8 bits)


class IvfPqError(IvfError):
    pass


def _lib():
    lib = load_library()
    if not getattr(lib, "_ivfpq_ready", False):
        for name, (res, args) in PROTOS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        lib._ivfpq_ready = True
    return lib


def _check(lib, rc: int) -> None:
    if rc != 0:
        raise IvfPqError(f"ivfpq_ann error {rc}: {lib.ivfpq_last_error().decode()}")


class FaissIvfPq:
    """`IVF<nlist>,PQ<M>` (8-bit codes, residuals) in an id map, resident in HBM: train() or load() the coarse quantizer
    and the codebooks, add() rows, search().  The rows themselves are not kept."""

    def __init__(self, handle, metric: DistanceMetric, d: int, nlist: int, M: int):
        self._h, self.metric, self.d, self.nlist, self.M = handle, DistanceMetric(metric), d, nlist, M

    @classmethod
    def train(cls, metric: DistanceMetric, nlist: int, M: int, train_vectors: np.ndarray, *, niter: int = 0, seed: int = 1,
              device: int = 0):
        """Deterministic k-means of the cells, then of the M codebooks on the residuals (niter: 0 = 20 rounds, -1 = the
        initial picks; it serves both)."""
        lib = _lib()
        v = _rows(train_vectors)
        h = C.c_void_p()
        _check(lib, lib.ivfpq_index_train(device, int(metric), v.shape[1], nlist, M, v.shape[0], v.ctypes.data, niter, seed,
                                          C.byref(h)))
        return cls(h, metric, v.shape[1], nlist, M)

    @classmethod
    def load(cls, metric: DistanceMetric, centroids: np.ndarray, codebooks: np.ndarray, *, device: int = 0):
        """centroids [nlist, d]; codebooks [M, 256, d / M]."""
        lib = _lib()
        c = _rows(centroids)
        cb = np.ascontiguousarray(codebooks, np.float32)
        if cb.ndim != 3 or cb.shape[1] != KSUB or cb.shape[0] * cb.shape[2] != c.shape[1]:
            raise ValueError(f"expected codebooks of shape [M, {KSUB}, {c.shape[1]} / M], got {cb.shape}")
        h = C.c_void_p()
        _check(lib, lib.ivfpq_index_load(device, int(metric), c.shape[1], c.shape[0], cb.shape[0], c.ctypes.data, cb.ctypes.data,
                                         C.byref(h)))
        return cls(h, metric, c.shape[1], c.shape[0], cb.shape[0])

    @property
    def n(self) -> int:
        n = C.c_int64()
        lib = _lib()
        _check(lib, lib.ivfpq_index_info(self._h, C.byref(n), None, None, None, None))
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
        _check(lib, lib.ivfpq_index_add(self._h, v.shape[0], v.ctypes.data, idp.ctypes.data if idp is not None else None))

    def search(self, queries: np.ndarray, k: int, nprobe: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(ids [nq, k], distances [nq, k], counts [nq]): the k nearest codes of the nprobe nearest cells' lists, ascending
        by (distance, id); counts may fall short of k."""
        lib = _lib()
        q = _rows(queries, self.d)
        nq = q.shape[0]
        dist = np.zeros((nq, k), np.float32)
        ids = np.zeros((nq, k), np.int64)
        cnt = np.zeros(nq, np.int32)
        _check(lib, lib.ivfpq_search(self._h, nq, q.ctypes.data, k, nprobe, dist.ctypes.data, ids.ctypes.data, cnt.ctypes.data))
        return ids, dist, cnt

    def centroids(self) -> np.ndarray:
        out = np.empty((self.nlist, self.d), np.float32)
        lib = _lib()
        _check(lib, lib.ivfpq_index_get_centroids(self._h, out.ctypes.data))
        return out

    def codebooks(self) -> np.ndarray:
        """fp32 [M, 256, d / M]."""
        out = np.empty((self.M, KSUB, self.d // self.M), np.float32)
        lib = _lib()
        _check(lib, lib.ivfpq_index_get_codebooks(self._h, out.ctypes.data))
        return out

    def codes(self) -> np.ndarray:
        """uint8 [n, M], the rows in the order they were added."""
        out = np.empty((self.n, self.M), np.uint8)
        lib = _lib()
        _check(lib, lib.ivfpq_index_get_codes(self._h, out.ctypes.data))
        return out

    def list_sizes(self) -> np.ndarray:
        out = np.empty(self.nlist, np.int64)
        lib = _lib()
        _check(lib, lib.ivfpq_index_list_sizes(self._h, out.ctypes.data))
        return out

    def assignment(self) -> Tuple[np.ndarray, np.ndarray]:
        """(ids [n], cells [n]) of the rows in the order they were added."""
        n = self.n
        ids, cells = np.empty(n, np.int64), np.empty(n, np.int32)
        lib = _lib()
        _check(lib, lib.ivfpq_index_get_assignment(self._h, ids.ctypes.data, cells.ctypes.data))
        return ids, cells

    def last_probes(self) -> np.ndarray:
        """The cells the last search probed, nearest first: int32 [nq, nprobe] (nprobe after clamping to nlist)."""
        nq, npr = C.c_int32(), C.c_int32()
        lib = _lib()
        _check(lib, lib.ivfpq_last_probes(self._h, C.byref(nq), C.byref(npr), None))
        out = np.empty((nq.value, npr.value), np.int32)
        _check(lib, lib.ivfpq_last_probes(self._h, None, None, out.ctypes.data))
        return out

    def last_stats(self) -> dict:
        rows, rounds = C.c_int64(), C.c_int32()
        a, b, s = C.c_float(), C.c_float(), C.c_float()
        lib = _lib()
        _check(lib, lib.ivfpq_last_stats(self._h, C.byref(rows), C.byref(rounds), C.byref(a), C.byref(b), C.byref(s)))
        return {"rows_scanned": rows.value, "rounds": rounds.value, "coarse_ms": a.value, "scan_ms": b.value, "select_ms": s.value}

    def bytes_per_row(self) -> int:
        """Device bytes per row: the code in the order added and in its list, the id (twice: as added and sorted), the
        cell and the slot's rank (padding of a list's last block aside)."""
        return 2 * self.M + 8 + 8 + 4 + 4

    def close(self) -> None:
        if self._h:
            _lib().ivfpq_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_FACTORY = re.compile(r"IVF(\d+),(?:(Flat)|PQ(\d+)(?:x8)?)")


class IndexSpec:
    """What index_factory returns: an untrained index.  train() yields the trained, empty FaissIvfFlat / FaissIvfPq."""

    def __init__(self, dimension: int, metric: DistanceMetric, nlist: int, M: Optional[int], factory_string: str):
        self.dimension, self.metric, self.nlist, self.M, self.factory_string = dimension, DistanceMetric(metric), nlist, M, factory_string

    @property
    def index_class(self):
        return FaissIvfFlat if self.M is None else FaissIvfPq

    def train(self, vectors: np.ndarray, niter: int = 0, seed: int = 1, *, device: int = 0):
        v = _rows(vectors, self.dimension)
        if self.M is None:
            return FaissIvfFlat.train(self.metric, self.nlist, v, niter=niter, seed=seed, device=device)
        return FaissIvfPq.train(self.metric, self.nlist, self.M, v, niter=niter, seed=seed, device=device)


def index_factory(dimension: int, factory_string: str, metric: DistanceMetric) -> IndexSpec:
    """Faiss's index_factory for `IVF<nlist>,Flat`, `IVF<nlist>,PQ<M>` and `IVF<nlist>,PQ<M>x8`."""
    m = _FACTORY.fullmatch(factory_string) if isinstance(factory_string, str) else None
    if m is None:
        raise ValueError(f"index_factory: unsupported factory string {factory_string!r} "
                         "(IVF<nlist>,Flat, IVF<nlist>,PQ<M> and IVF<nlist>,PQ<M>x8 are served)")
    return IndexSpec(int(dimension), metric, int(m.group(1)), None if m.group(2) else int(m.group(3)), factory_string)


def training_set_size(n: int, sample_rate: float) -> int:
    """FaissIndexer.scala:86: Math.min(datasetSize, Math.round(datasetSize * sampleRate)) -- a Float product, rounded half up."""
    return min(n, int(np.floor(np.float64(np.float32(n) * np.float32(sample_rate)) + 0.5)))


def build_faiss_index(vectors: np.ndarray, ids: Sequence[int], sample_rate: float, factory_string: str, metric: DistanceMetric,
                      *, niter: int = 0, seed: int = 1, device: int = 0):
    """FaissIndexer.buildAndWriteFaissIndex (:82-92) without the write: index_factory, train on the first trainingSetSize
    rows, add_with_ids all rows."""
    v = _rows(vectors)
    spec = index_factory(v.shape[1], factory_string, metric)
    index = spec.train(v[:training_set_size(v.shape[0], sample_rate)], niter, seed, device=device)
    index.add(v, ids)
    return index
