"""ctypes binding of include/ivfsq_ann.h (Faiss `IVF<nlist>,SQ8`): inverted lists of one byte per component, scanned on
the matrix cores; Faiss's index_factory for that string and the reference's index build over it.

Reference (paths relative to the reference's ann/src/main/):
  scala/com/twitter/ann/faiss/FaissIndexer.scala:82-92                      index_factory -> train -> add_with_ids
  scala/com/twitter/ann/dataflow/offline/ANNIndexBuilderBeamJob.scala:143-144  the factory string "determines the ANN
                                                                             algorithm and compression"
FaissQueryable (ivf_ann.py) works over FaissIvfSq8 unchanged: it needs search() alone.  The index cannot be saved, put
into a ShardSet, refined or given an HNSW quantizer: its FAISS_KIND is 0, which those modules refuse.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import Optional, Sequence, Tuple

import numpy as np

from .. import binding as _binding
from .. import hnsw_quantizer, ivfpq_ann
from ..dense_ann import DistanceMetric
from ..ivf_ann import FaissParams, FaissQueryable, IvfError, _IvfFamilyIndex, _rows  # noqa: F401
from ..simclusters_ann import load_library

_P = C.POINTER
PROTOS = {
    "ivfsq_last_error": (C.c_char_p, []),
    "ivfsq_index_train": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_uint64,
                                    _P(C.c_void_p)]),
    "ivfsq_index_load": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, _P(C.c_void_p)]),
    "ivfsq_index_add": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ivfsq_search": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ivfsq_index_info": (C.c_int, [C.c_void_p, _P(C.c_int64), _P(C.c_int32), _P(C.c_int32), _P(C.c_int32)]),
    "ivfsq_index_get_centroids": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ivfsq_index_get_ranges": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ivfsq_index_list_sizes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ivfsq_index_get_assignment": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ivfsq_index_get_codes": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "ivfsq_last_probes": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), C.c_void_p]),
    "ivfsq_last_stats": (C.c_int, [C.c_void_p, _P(C.c_int64), _P(C.c_int32), _P(C.c_float), _P(C.c_float), _P(C.c_float)]),
    "ivfsq_index_destroy": (C.c_int, [C.c_void_p]),
}


class IvfSqError(IvfError):
    pass


_lib = _binding.binder(PROTOS, "ivfsq", load_library)
_check = _binding.checker(IvfSqError, "ivfsq_ann", "ivfsq_last_error")


class FaissIvfSq8(_IvfFamilyIndex):
    """`IVF<nlist>,SQ8` (QT_8bit, the rows themselves, not residuals) in an id map, resident in HBM: train() or load() the
    coarse quantizer and the ranges, add() rows, search().  The rows themselves are not kept."""

    _prefix, _destroy, _info_fields, FAISS_KIND = "ivfsq", "ivfsq_index_destroy", 3, 0
    _lib, _check = staticmethod(_lib), staticmethod(_check)

    def __init__(self, handle, metric: DistanceMetric, d: int, nlist: int):
        self._h, self.metric, self.d, self.nlist = handle, DistanceMetric(metric), d, nlist

    @classmethod
    def _from_handle(cls, handle):
        _, (d, metric, nlist) = cls._read_info(handle)
        return cls(handle, DistanceMetric(metric), d, nlist)

    @classmethod
    def train(cls, metric: DistanceMetric, nlist: int, train_vectors: np.ndarray, *, niter: int = 0, seed: int = 1, device: int = 0):
        """The centroids of FaissIvfFlat.train over the same arguments, and per component the minimum and maximum of the
        prepared training rows."""
        lib = _lib()
        v = _rows(train_vectors)
        h = C.c_void_p()
        _check(lib, lib.ivfsq_index_train(device, int(metric), v.shape[1], nlist, v.shape[0], v.ctypes.data, niter, seed, C.byref(h)))
        return cls(h, metric, v.shape[1], nlist)

    @classmethod
    def load(cls, metric: DistanceMetric, centroids: np.ndarray, vmin: np.ndarray, vdiff: np.ndarray, *, device: int = 0):
        """centroids [nlist, d]; vmin and vdiff [d] (finite, vdiff >= 0)."""
        lib = _lib()
        c = _rows(centroids)
        lo, df = np.ascontiguousarray(vmin, np.float32), np.ascontiguousarray(vdiff, np.float32)
        if lo.shape != (c.shape[1],) or df.shape != (c.shape[1],):
            raise ValueError(f"expected vmin and vdiff of shape [{c.shape[1]}], got {lo.shape} and {df.shape}")
        h = C.c_void_p()
        _check(lib, lib.ivfsq_index_load(device, int(metric), c.shape[1], c.shape[0], c.ctypes.data, lo.ctypes.data, df.ctypes.data,
                                         C.byref(h)))
        return cls(h, metric, c.shape[1], c.shape[0])

    def ranges(self) -> Tuple[np.ndarray, np.ndarray]:
        """(vmin [d], vdiff [d]), fp32; step = vdiff / 255."""
        vmin, vdiff = np.empty(self.d, np.float32), np.empty(self.d, np.float32)
        self._call("_index_get_ranges", vmin.ctypes.data, vdiff.ctypes.data)
        return vmin, vdiff

    def codes(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """uint8 [count, d]: the codes of rows [first, first + count) in the order they were added (default: all)."""
        m = self.n - first if count is None else count
        out = np.empty((max(m, 0), self.d), np.uint8)
        self._call("_index_get_codes", first, m, out.ctypes.data)
        return out

    def bytes_per_row(self) -> int:
        """Device bytes per row: the code in the order added and in its list, |xhat|^2 and the bias, the id (as added and
        sorted), the cell and the slot's rank (padding of a list's last block aside)."""
        return 2 * self.d + 4 + 4 + 8 + 8 + 4 + 4


_FACTORY = re.compile(r"IVF(\d+),SQ8")


class Sq8IndexSpec:
    """What index_factory returns for `IVF<nlist>,SQ8`: an untrained index.  train() yields the trained, empty FaissIvfSq8."""

    M = None

    def __init__(self, dimension: int, metric: DistanceMetric, nlist: int, factory_string: str):
        self.dimension, self.metric, self.nlist, self.factory_string = dimension, DistanceMetric(metric), nlist, factory_string

    @property
    def index_class(self):
        return FaissIvfSq8

    def train(self, vectors: np.ndarray, niter: int = 0, seed: int = 1, *, device: int = 0):
        return FaissIvfSq8.train(self.metric, self.nlist, _rows(vectors, self.dimension), niter=niter, seed=seed, device=device)


def index_factory(dimension: int, factory_string: str, metric: DistanceMetric):
    """Faiss's index_factory: `IVF<nlist>,SQ8` is served here; every other string goes to hnsw_quantizer.index_factory
    (and from there to the older factories), whose refusals are this one's."""
    m = _FACTORY.fullmatch(factory_string) if isinstance(factory_string, str) else None
    if m is None:
        return hnsw_quantizer.index_factory(dimension, factory_string, metric)
    return Sq8IndexSpec(int(dimension), metric, int(m.group(1)), factory_string)


def build_faiss_index(vectors: np.ndarray, ids: Sequence[int], sample_rate: float, factory_string: str, metric: DistanceMetric,
                      *, niter: int = 0, seed: int = 1, device: int = 0):
    """FaissIndexer.buildAndWriteFaissIndex (:82-92) without the write, over this module's index_factory: train on the first
    trainingSetSize rows, add_with_ids all rows."""
    v = _rows(vectors)
    spec = index_factory(v.shape[1], factory_string, metric)
    index = spec.train(v[:ivfpq_ann.training_set_size(v.shape[0], sample_rate)], niter, seed, device=device)
    index.add(v, ids)
    return index
