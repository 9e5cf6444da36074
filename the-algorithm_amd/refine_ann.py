"""ctypes binding of include/refine_ann.h (`<base>,RFlat` / `<base>,Refine(Flat)`): the rows kept beside an IVF-PQ or OPQ
index, whose k * k_factor candidates are re-ranked by their true distances; Faiss's index_factory for those strings, and the
reference's index build over it.

Reference (paths relative to the reference's ann/src/main/):
  scala/com/twitter/ann/faiss/FaissIndexer.scala:82-92            index_factory -> train -> add_with_ids
  thrift/com/twitter/ann/common/ann_common.thrift:49-50           "How many times more neighbours are requested from
                                                                  underlying index by IndexRefine"
k_factor is a field of the Faiss index, written with it: the builder sets it, no runtime parameter carries it.
FaissQueryable (ivf_ann.py) works over FaissRefineFlat unchanged: it needs search() alone.
Not here: saving and loading (faiss_files has no row section), JNI, a refine index as the coarse quantizer.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import Optional, Sequence, Tuple

import numpy as np

from . import binding as _binding
from . import ivfpq_ann, opq_ann
from .dense_ann import DistanceMetric
from .ivf_ann import IvfError, _rows
from .simclusters_ann import load_library

_P = C.POINTER
_SEARCH = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]
_OUT = [C.c_void_p, C.c_void_p, C.c_void_p]
PROTOS = {
    "refine_last_error": (C.c_char_p, []),
    "refine_index_wrap_ivfpq": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_void_p)]),
    "refine_index_wrap_opq": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_void_p)]),
    "refine_index_add": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "refine_search": (C.c_int, _SEARCH + _OUT),
    "refine_search_with_k_factor": (C.c_int, _SEARCH + [C.c_int32] + _OUT),
    "refine_index_set_k_factor": (C.c_int, [C.c_void_p, C.c_int32]),
    "refine_index_info": (C.c_int, [C.c_void_p, _P(C.c_int64), _P(C.c_int32), _P(C.c_int32), _P(C.c_int32), _P(C.c_int32)]),
    "refine_index_base": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_void_p)]),
    "refine_last_candidates": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), C.c_void_p, C.c_void_p]),
    "refine_index_get_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "refine_last_stats": (C.c_int, [C.c_void_p, _P(C.c_float), _P(C.c_float)]),
    "refine_index_destroy": (C.c_int, [C.c_void_p]),
}

BASE_IVFPQ, BASE_OPQ = 0, 1
MAX_K_FACTOR = 1024
MAX_CANDIDATES = 1024  # k * k_factor: the most the base answers


class RefineError(IvfError):
    pass


_lib = _binding.binder(PROTOS, "refine", load_library)
_check = _binding.checker(RefineError, "refine_ann", "refine_last_error")

_WRAP = {ivfpq_ann.FaissIvfPq.FAISS_KIND: "refine_index_wrap_ivfpq", opq_ann.FaissOpqIvfPq.FAISS_KIND: "refine_index_wrap_opq"}


class FaissRefineFlat(_binding.Handle):
    """`<base>,RFlat` in an id map, resident in HBM: wrap() a trained, empty FaissIvfPq or FaissOpqIvfPq, add() rows (they go
    to the base and, as fp16, to the store), search().  The handle owns the base; `base` stays usable for its exports."""

    _destroy, _lib = "refine_index_destroy", staticmethod(_lib)

    def __init__(self, handle, base):
        base._disown()  # the C handle owns the base: it is destroyed with the refined index
        self._h, self.base = handle, base
        self.metric = base.metric
        self.d = getattr(base, base._row_dim)  # the dimension of rows and queries
        self.nlist, self.M = base.nlist, base.M

    @classmethod
    def wrap(cls, base, k_factor: int = 1):
        """Takes the base over (its own close() becomes a no-op); the base must hold no row yet."""
        fn = _WRAP.get(getattr(base, "FAISS_KIND", None))
        if fn is None:
            raise TypeError(f"a refined index wraps a FaissIvfPq or a FaissOpqIvfPq, not {type(base).__name__}")
        base._owning()  # a base that another index has wrapped or adopted is refused before the library sees it
        lib = _lib()
        h = C.c_void_p()
        _check(lib, getattr(lib, fn)(base._h, int(k_factor), C.byref(h)))
        return cls(h, base)

    def _closed(self) -> None:
        self.base._h = None  # it went with the refined index

    def _info(self):
        n, d, metric, kf, kind = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        lib = _lib()
        _check(lib, lib.refine_index_info(self._h, C.byref(n), C.byref(d), C.byref(metric), C.byref(kf), C.byref(kind)))
        return n.value, d.value, metric.value, kf.value, kind.value

    @property
    def n(self) -> int:
        return self._info()[0]

    @property
    def k_factor(self) -> int:
        return self._info()[3]

    @k_factor.setter
    def k_factor(self, value: int) -> None:
        lib = _lib()
        _check(lib, lib.refine_index_set_k_factor(self._h, int(value)))

    @property
    def base_kind(self) -> int:
        return self._info()[4]

    def add(self, vectors: np.ndarray, ids: Optional[Sequence[int]] = None) -> None:
        """add_with_ids.  ids on every call or on none (ids = positions in the order added)."""
        lib = _lib()
        v = _rows(vectors, self.d)
        idp = _binding.ids_or_none(ids, v.shape[0])
        _check(lib, lib.refine_index_add(self._h, v.shape[0], v.ctypes.data, _binding.ptr(idp)))

    def search(self, queries: np.ndarray, k: int, nprobe: int, k_factor: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(ids [nq, k], distances [nq, k], counts [nq]): the k nearest by true distance of the base's k * k_factor
        candidates, ascending by (distance, id).  k_factor: that of this call (default: the index's)."""
        lib = _lib()
        q = _rows(queries, self.d)
        nq = q.shape[0]
        ids, dist, cnt = _binding.result_triple(nq, k)
        if k_factor is None:
            _check(lib, lib.refine_search(self._h, nq, q.ctypes.data, k, nprobe, dist.ctypes.data, ids.ctypes.data, cnt.ctypes.data))
        else:
            _check(lib, lib.refine_search_with_k_factor(self._h, nq, q.ctypes.data, k, nprobe, int(k_factor), dist.ctypes.data,
                                                        ids.ctypes.data, cnt.ctypes.data))
        return ids, dist, cnt

    def last_candidates(self) -> Tuple[np.ndarray, np.ndarray]:
        """(positions int32 [nq, k * k_factor], counts [nq]) of the last search: what the base handed to the re-rank, as
        add-order positions, best first by the base's order; -1 past the count."""
        nq, width = C.c_int32(), C.c_int32()
        lib = _lib()
        _check(lib, lib.refine_last_candidates(self._h, C.byref(nq), C.byref(width), None, None))
        pos = np.full((nq.value, width.value), -1, np.int32)
        cnt = np.zeros(nq.value, np.int32)
        _check(lib, lib.refine_last_candidates(self._h, None, None, pos.ctypes.data, cnt.ctypes.data))
        return pos, cnt

    def rows(self, row0: int = 0, m: Optional[int] = None) -> np.ndarray:
        """The stored rows [row0, row0 + m) in the order added: float16 [m, d]."""
        if m is None:
            m = self.n - row0
        out = np.empty((m, self.d), np.float16)
        lib = _lib()
        _check(lib, lib.refine_index_get_rows(self._h, row0, m, out.ctypes.data))
        return out

    def last_stats(self) -> dict:
        a, b = C.c_float(), C.c_float()
        lib = _lib()
        _check(lib, lib.refine_last_stats(self._h, C.byref(a), C.byref(b)))
        return {"base_ms": a.value, "rerank_ms": b.value}

    def bytes_per_row(self) -> int:
        """Device bytes per row: the base's and the stored halves (padding to 8 halves aside)."""
        return self.base.bytes_per_row() + 2 * self.d


_SUFFIX = re.compile(r"(.*PQ\d+(?:x8)?),(?:RFlat|Refine\(Flat\))")


class RefineIndexSpec:
    """What index_factory returns for a `,RFlat` string: an untrained index.  train() yields the trained, empty
    FaissRefineFlat over the trained base."""

    index_class = FaissRefineFlat

    def __init__(self, base_spec, k_factor: int, factory_string: str):
        self.base_spec, self.k_factor, self.factory_string = base_spec, int(k_factor), factory_string
        self.dimension, self.metric = base_spec.dimension, base_spec.metric

    def train(self, vectors: np.ndarray, niter: int = 0, seed: int = 1, **kwargs):
        base = self.base_spec.train(vectors, niter, seed, **kwargs)
        try:
            return FaissRefineFlat.wrap(base, self.k_factor)
        except Exception:
            base.close()
            raise


def index_factory(dimension: int, factory_string: str, metric: DistanceMetric, k_factor: int = 1):
    """Faiss's index_factory for `<base>,RFlat` and `<base>,Refine(Flat)`, <base> being any string opq_ann.index_factory
    serves that ends in PQ<M>[x8]; every other string goes to opq_ann.index_factory unchanged (k_factor then has no
    meaning and must be 1)."""
    m = _SUFFIX.fullmatch(factory_string) if isinstance(factory_string, str) else None
    if m is None:
        if k_factor != 1:
            raise ValueError(f"index_factory: {factory_string!r} has no refinement: k_factor = {k_factor} cannot be set")
        return opq_ann.index_factory(dimension, factory_string, metric)
    if not 1 <= int(k_factor) <= MAX_K_FACTOR:
        raise ValueError(f"index_factory: {factory_string!r}: k_factor must be in 1..{MAX_K_FACTOR}, got {k_factor}")
    try:
        base = opq_ann.index_factory(dimension, m.group(1), metric)
    except ValueError as e:
        raise ValueError(f"index_factory: {factory_string!r}: the base is refused: {e}") from None
    return RefineIndexSpec(base, k_factor, factory_string)


def build_faiss_index(vectors: np.ndarray, ids: Sequence[int], sample_rate: float, factory_string: Optional[str] = None,
                      metric: DistanceMetric = DistanceMetric.Cosine, *, k_factor: int = 1, niter: int = 0, niter_opq: int = 0,
                      seed: int = 1, device: int = 0):
    """FaissIndexer.buildAndWriteFaissIndex (:82-92) without the write, over this module's index_factory: train on the
    first trainingSetSize rows, add_with_ids all rows.  No factory string: the default of faiss_index_bq_dataset.py."""
    v = _rows(vectors)
    if factory_string is None:
        factory_string = opq_ann.default_factory_string(v.shape[0], v.shape[1])
    spec = index_factory(v.shape[1], factory_string, metric, k_factor)
    head = v[:ivfpq_ann.training_set_size(v.shape[0], sample_rate)]
    base_spec = spec.base_spec if isinstance(spec, RefineIndexSpec) else spec
    if isinstance(base_spec, opq_ann.OpqIndexSpec):
        index = spec.train(head, niter, seed, niter_opq=niter_opq, device=device)
    else:
        index = spec.train(head, niter, seed, device=device)
    index.add(v, ids)
    return index
