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
from typing import Optional, Sequence

import numpy as np

from .dense_ann import DistanceMetric
from . import binding as _binding
from .ivf_ann import KIND_IVF_PQ as _KIND, FaissIvfFlat, IvfError, _IvfFamilyIndex, _rows
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


_lib = _binding.binder(PROTOS, "ivfpq", load_library)
_check = _binding.checker(IvfPqError, "ivfpq_ann", "ivfpq_last_error")


class _PqCodes:
    """The exports of the product quantiser, for FaissIvfPq and FaissOpqIvfPq (there `d` is the transform's d_out)."""

    def codebooks(self) -> np.ndarray:
        """fp32 [M, 256, d / M]."""
        out = np.empty((self.M, KSUB, self.d // self.M), np.float32)
        self._call("_index_get_codebooks", out.ctypes.data)
        return out

    def codes(self) -> np.ndarray:
        """uint8 [n, M], the rows in the order they were added."""
        out = np.empty((self.n, self.M), np.uint8)
        self._call("_index_get_codes", out.ctypes.data)
        return out

    def bytes_per_row(self) -> int:
        """Device bytes per row: the code in the order added and in its list, the id (twice: as added and sorted), the
        cell and the slot's rank (padding of a list's last block aside).  An OPQ matrix is per index, not per row."""
        return 2 * self.M + 8 + 8 + 4 + 4


class FaissIvfPq(_PqCodes, _IvfFamilyIndex):
    """`IVF<nlist>,PQ<M>` (8-bit codes, residuals) in an id map, resident in HBM: train() or load() the coarse quantizer
    and the codebooks, add() rows, search().  The rows themselves are not kept."""

    _prefix, _destroy, _info_fields, FAISS_KIND = "ivfpq", "ivfpq_index_destroy", 4, _KIND
    _lib, _check = staticmethod(_lib), staticmethod(_check)

    def __init__(self, handle, metric: DistanceMetric, d: int, nlist: int, M: int):
        self._h, self.metric, self.d, self.nlist, self.M = handle, DistanceMetric(metric), d, nlist, M

    @classmethod
    def _from_handle(cls, handle):
        _, (d, metric, nlist, M) = cls._read_info(handle)
        return cls(handle, DistanceMetric(metric), d, nlist, M)

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
