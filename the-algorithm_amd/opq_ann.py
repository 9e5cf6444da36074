"""ctypes binding of include/opq_ann.h (`OPQ<M>[_<dout>],IVF<nlist>,PQ<M>`): the learned rotation / projection in front of
the IVF-PQ index, Faiss's index_factory for the strings the device can serve with it, the factory string the reference
builds by default, and the reference's index build.

Reference (paths relative to the reference's ann/src/main/):
  python/dataflow/faiss_index_bq_dataset.py:178-188              the default factory string
  scala/com/twitter/ann/faiss/FaissIndexer.scala:82-92            index_factory -> train -> add_with_ids
  scala/com/twitter/ann/faiss/QueryableIndexAdapter.scala:43-65   Cosine: normalise, inner product, 1 - sim
FaissQueryable (ivf_ann.py) works over FaissOpqIvfPq unchanged: it needs search() alone.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import Optional, Sequence, Tuple

import numpy as np

from . import binding as _binding
from . import ivfpq_ann
from .dense_ann import DistanceMetric
from .ivf_ann import KIND_OPQ_IVF_PQ as _KIND, IvfError, _IvfFamilyIndex, _rows
from .simclusters_ann import load_library

_P = C.POINTER
PROTOS = {
    "opq_last_error": (C.c_char_p, []),
    "opq_index_train": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p,
                                  C.c_int32, C.c_int32, C.c_uint64, _P(C.c_void_p)]),
    "opq_index_load": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                 C.c_void_p, _P(C.c_void_p)]),
    "opq_index_add": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "opq_search": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "opq_transform": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "opq_index_info": (C.c_int, [C.c_void_p, _P(C.c_int64), _P(C.c_int32), _P(C.c_int32), _P(C.c_int32), _P(C.c_int32),
                                 _P(C.c_int32)]),
    "opq_index_get_matrix": (C.c_int, [C.c_void_p, C.c_void_p]),
    "opq_training_errors": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_int32)]),
    "opq_training_stats": (C.c_int, [C.c_void_p, _P(C.c_float), _P(C.c_float), _P(C.c_float), _P(C.c_float), _P(C.c_float)]),
    "opq_index_get_centroids": (C.c_int, [C.c_void_p, C.c_void_p]),
    "opq_index_get_codebooks": (C.c_int, [C.c_void_p, C.c_void_p]),
    "opq_index_get_codes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "opq_index_list_sizes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "opq_index_get_assignment": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "opq_last_probes": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), C.c_void_p]),
    "opq_last_stats": (C.c_int, [C.c_void_p, _P(C.c_int64), _P(C.c_int32), _P(C.c_float), _P(C.c_float), _P(C.c_float),
                                 _P(C.c_float)]),
    "opq_index_destroy": (C.c_int, [C.c_void_p]),
    "opq_procrustes": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "opq_debug_correlation": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
}

KSUB = ivfpq_ann.KSUB


class OpqError(IvfError):
    pass


_lib = _binding.binder(PROTOS, "opq", load_library)
_check = _binding.checker(OpqError, "opq_ann", "opq_last_error")


def procrustes(C_: np.ndarray) -> np.ndarray:
    """The matrix A [d_out, d_in] with orthonormal rows that maximises tr(A C) for C [d_in, d_out] (float64).  Host only."""
    c = np.ascontiguousarray(C_, np.float64)
    if c.ndim != 2 or c.shape[1] > c.shape[0]:
        raise ValueError(f"expected C of shape [d_in, d_out] with d_out <= d_in, got {c.shape}")
    out = np.empty((c.shape[1], c.shape[0]), np.float64)
    lib = _lib()
    _check(lib, lib.opq_procrustes(c.shape[0], c.shape[1], c.ctypes.data, out.ctypes.data))
    return out


def debug_correlation(x: np.ndarray, y_hat: np.ndarray, *, device: int = 0) -> np.ndarray:
    """Test seam: X^T Y^ [d_in, d_out] in float64 by the correlation kernels of the training."""
    xx, yy = _rows(x), _rows(y_hat)
    if xx.shape[0] != yy.shape[0]:
        raise ValueError("one row of y_hat per row of x")
    out = np.empty((xx.shape[1], yy.shape[1]), np.float64)
    lib = _lib()
    _check(lib, lib.opq_debug_correlation(device, xx.shape[0], xx.shape[1], yy.shape[1], xx.ctypes.data, yy.ctypes.data,
                                          out.ctypes.data))
    return out


class FaissOpqIvfPq(ivfpq_ann._PqCodes, _IvfFamilyIndex):
    """`OPQ<M>_<d_out>,IVF<nlist>,PQ<M>` in an id map, resident in HBM: train() or load() the matrix, the coarse quantizer
    and the codebooks, add() rows of d_in components, search().  Rows are transformed on the device and not kept."""

    _prefix, _destroy, _info_fields, FAISS_KIND = "opq", "opq_index_destroy", 5, _KIND
    _row_dim, _STATS = "d_in", _IvfFamilyIndex._STATS + ("transform_ms",)
    _lib, _check = staticmethod(_lib), staticmethod(_check)

    def __init__(self, handle, metric: DistanceMetric, d_in: int, d_out: int, nlist: int, M: int):
        self._h, self.metric, self.d_in, self.d_out, self.nlist, self.M = handle, DistanceMetric(metric), d_in, d_out, nlist, M
        self.d = d_out  # the dimension of what the exports describe (centroids, codebooks), as FaissIvfPq.d

    @classmethod
    def _from_handle(cls, handle):
        _, (d_in, d_out, metric, nlist, M) = cls._read_info(handle)
        return cls(handle, DistanceMetric(metric), d_in, d_out, nlist, M)

    @classmethod
    def train(cls, metric: DistanceMetric, nlist: int, M: int, d_out: int, train_vectors: np.ndarray, *, niter: int = 0,
              niter_opq: int = 0, seed: int = 1, device: int = 0):
        """The matrix by niter_opq rounds (0 = 50) of product quantiser / Procrustes on the first 65536 rows, then the
        cells and codebooks on the transformed rows (niter as FaissIvfPq.train).  Deterministic."""
        lib = _lib()
        v = _rows(train_vectors)
        h = C.c_void_p()
        _check(lib, lib.opq_index_train(device, int(metric), v.shape[1], d_out, nlist, M, v.shape[0], v.ctypes.data, niter,
                                        niter_opq, seed, C.byref(h)))
        return cls(h, metric, v.shape[1], d_out, nlist, M)

    @classmethod
    def load(cls, metric: DistanceMetric, matrix: np.ndarray, centroids: np.ndarray, codebooks: np.ndarray, *, device: int = 0):
        """matrix [d_out, d_in] (kept as given); centroids [nlist, d_out]; codebooks [M, 256, d_out / M]."""
        lib = _lib()
        a = _rows(matrix)
        c = _rows(centroids, a.shape[0])
        cb = np.ascontiguousarray(codebooks, np.float32)
        if cb.ndim != 3 or cb.shape[1] != KSUB or cb.shape[0] * cb.shape[2] != c.shape[1]:
            raise ValueError(f"expected codebooks of shape [M, {KSUB}, {c.shape[1]} / M], got {cb.shape}")
        h = C.c_void_p()
        _check(lib, lib.opq_index_load(device, int(metric), a.shape[1], a.shape[0], c.shape[0], cb.shape[0], a.ctypes.data,
                                       c.ctypes.data, cb.ctypes.data, C.byref(h)))
        return cls(h, metric, a.shape[1], a.shape[0], c.shape[0], cb.shape[0])

    def transform(self, x: np.ndarray) -> np.ndarray:
        """What added rows and queries become before the inner index rounds them to fp16: fp32 [n, d_out] (Cosine: the
        rows are normalised first)."""
        lib = _lib()
        v = _rows(x, self.d_in)
        out = np.empty((v.shape[0], self.d_out), np.float32)
        _check(lib, lib.opq_transform(self._h, v.shape[0], v.ctypes.data, out.ctypes.data))
        return out

    def matrix(self) -> np.ndarray:
        """fp32 [d_out, d_in]."""
        out = np.empty((self.d_out, self.d_in), np.float32)
        lib = _lib()
        _check(lib, lib.opq_index_get_matrix(self._h, out.ctypes.data))
        return out

    def training_errors(self) -> np.ndarray:
        """err[t] = mean ||Y - Y^||^2 of training round t (float64; empty for a loaded index)."""
        cnt = C.c_int32()
        lib = _lib()
        _check(lib, lib.opq_training_errors(self._h, None, C.byref(cnt)))
        out = np.empty(cnt.value, np.float64)
        _check(lib, lib.opq_training_errors(self._h, out.ctypes.data, None))
        return out

    def training_stats(self) -> dict:
        v = [C.c_float() for _ in range(5)]
        lib = _lib()
        _check(lib, lib.opq_training_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(["transform_ms", "pq_ms", "correlation_ms", "procrustes_ms", "inner_ms"], [x.value for x in v]))


_FACTORY = re.compile(r"OPQ(\d+)(?:_(\d+))?,IVF(\d+),PQ(\d+)(?:x8)?")


class OpqIndexSpec:
    """What index_factory returns for an OPQ string: an untrained index.  train() yields the trained, empty FaissOpqIvfPq."""

    index_class = FaissOpqIvfPq

    def __init__(self, dimension: int, metric: DistanceMetric, d_out: int, nlist: int, M: int, factory_string: str):
        self.dimension, self.metric, self.d_out, self.nlist, self.M = dimension, DistanceMetric(metric), d_out, nlist, M
        self.factory_string = factory_string

    def train(self, vectors: np.ndarray, niter: int = 0, seed: int = 1, *, niter_opq: int = 0, device: int = 0):
        v = _rows(vectors, self.dimension)
        return FaissOpqIvfPq.train(self.metric, self.nlist, self.M, self.d_out, v, niter=niter, niter_opq=niter_opq, seed=seed,
                                   device=device)


def index_factory(dimension: int, factory_string: str, metric: DistanceMetric):
    """Faiss's index_factory for `OPQ<M>,IVF<nlist>,PQ<M>[x8]` (d_out = dimension) and `OPQ<M>_<dout>,IVF<nlist>,PQ<M>[x8]`;
    every other string goes to ivfpq_ann.index_factory unchanged."""
    m = _FACTORY.fullmatch(factory_string) if isinstance(factory_string, str) else None
    if m is None:
        return ivfpq_ann.index_factory(dimension, factory_string, metric)
    dimension = int(dimension)
    M_opq, d_out, nlist, M = int(m.group(1)), int(m.group(2)) if m.group(2) else dimension, int(m.group(3)), int(m.group(4))

    def refuse(why):
        return ValueError(f"index_factory: {factory_string!r} at dimension {dimension}: {why}")

    if M_opq != M:
        raise refuse(f"OPQ{M_opq} in front of PQ{M}: the two numbers of sub-quantizers must agree")
    if d_out > dimension:
        raise refuse(f"the transform's output dimension {d_out} exceeds the input dimension")
    if M < 1 or d_out % M:
        raise refuse(f"M = {M} does not divide the transform's output dimension {d_out}")
    if not 16 <= dimension <= 1024:
        raise refuse("the input dimension must be in 16..1024")
    if d_out < 16 or d_out > 512 or d_out % 16 or M < 4 or M > 64 or M % 4 or not 1 <= nlist <= 65536:
        raise refuse(f"IVF{nlist},PQ{M} at dimension {d_out} is a shape the IVF-PQ index does not serve "
                     "(dimension a multiple of 16 in 16..512, M a multiple of 4 in 4..64, nlist in 1..65536)")
    return OpqIndexSpec(dimension, metric, d_out, nlist, M, factory_string)


def default_factory_string(n: int, dimension: int) -> str:
    """faiss_index_bq_dataset.py:178-188: M = 48, the output dimension the largest multiple of M within the dimension (named
    only when it differs), one cell per 20 rows."""
    M = 48
    d_out = (dimension // M) * M
    prefix = f"OPQ{M}_{d_out}" if d_out != dimension else f"OPQ{M}"
    return f"{prefix},IVF{n // 20},PQ{M}"


def build_faiss_index(vectors: np.ndarray, ids: Sequence[int], sample_rate: float, factory_string: Optional[str] = None,
                      metric: DistanceMetric = DistanceMetric.Cosine, *, niter: int = 0, niter_opq: int = 0, seed: int = 1,
                      device: int = 0):
    """FaissIndexer.buildAndWriteFaissIndex (:82-92) without the write, with the default factory string of
    faiss_index_bq_dataset.py when none is given: index_factory, train on the first trainingSetSize rows, add_with_ids
    all rows."""
    v = _rows(vectors)
    if factory_string is None:
        factory_string = default_factory_string(v.shape[0], v.shape[1])
    spec = index_factory(v.shape[1], factory_string, metric)
    head = v[:ivfpq_ann.training_set_size(v.shape[0], sample_rate)]
    if isinstance(spec, OpqIndexSpec):
        index = spec.train(head, niter, seed, niter_opq=niter_opq, device=device)
    else:
        index = spec.train(head, niter, seed, device=device)
    index.add(v, ids)
    return index
