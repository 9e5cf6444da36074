"""ctypes binding of include/polysemous_ann.h: polysemous training of the IVF-PQ and OPQ indexes, the Hamming-filtered search
(Faiss's `ht`), Faiss's index_factory with its polysemous default, and the reference's queryable with `ht` passed through.

Reference (paths relative to the reference's ann/src/main/):
  thrift/com/twitter/ann/common/ann_common.thrift:41-56           FaissRuntimeParam: nprobe and ht are served here
  scala/com/twitter/ann/faiss/FaissCommon.scala:11-37             FaissParams <-> FaissRuntimeParam
  scala/com/twitter/ann/faiss/FaissIndexer.scala:82-92            index_factory -> train -> add_with_ids
  python/dataflow/faiss_index_bq_dataset.py:178-188              the default factory string, a polysemous index in Faiss
Faiss is not vendored in the reference: that index_factory trains `PQ<M>` polysemous unless it ends in `np`, and Faiss's
permutation and filter themselves, are UNPINNED.  ivfpq_ann.index_factory, opq_ann.index_factory and ivf_ann.FaissQueryable
are untouched: they keep training plain codes and refusing `ht`.  `ht` through refine_ann and the JNI methods are not built.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import binding as _binding
from . import ivfpq_ann, opq_ann
from .dense_ann import DistanceMetric
from .ivf_ann import MAX_COSINE_DISTANCE, FaissParams, FaissQueryable, IvfError, _rows
from .ivfpq_ann import KSUB, FaissIvfPq
from .opq_ann import FaissOpqIvfPq
from .simclusters_ann import load_library

_P = C.POINTER
_SEARCH_HT = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
PROTOS = {
    "polysemous_last_error": (C.c_char_p, []),
    "polysemous_optimize_codebook": (C.c_int, [C.c_int32, C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p, _P(C.c_double),
                                               _P(C.c_double)]),
    "ivfpq_index_train_polysemous": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p,
                                               C.c_int32, C.c_uint64, C.c_int64, _P(C.c_void_p)]),
    "ivfpq_index_is_polysemous": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "ivfpq_search_ht": (C.c_int, _SEARCH_HT),
    "ivfpq_last_query_codes": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), C.c_void_p]),
    "ivfpq_last_ht_stats": (C.c_int, [C.c_void_p, _P(C.c_int64)]),
    "opq_index_train_polysemous": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p,
                                             C.c_int32, C.c_int32, C.c_uint64, C.c_int64, _P(C.c_void_p)]),
    "opq_index_is_polysemous": (C.c_int, [C.c_void_p, _P(C.c_int32)]),
    "opq_search_ht": (C.c_int, _SEARCH_HT),
    "opq_last_query_codes": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), C.c_void_p]),
    "opq_last_ht_stats": (C.c_int, [C.c_void_p, _P(C.c_int64)]),
}

DEFAULT_ANNEAL_ITERS = 500000
_MASK = (1 << 64) - 1


class PolysemousError(IvfError):
    pass


_lib = _binding.binder(PROTOS, "polysemous", load_library, also=(ivfpq_ann._lib, opq_ann._lib))
_check = _binding.checker(PolysemousError, "polysemous_ann", None)


def mix64(x: int) -> int:
    """The 64-bit finaliser the library draws from."""
    x &= _MASK
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & _MASK
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & _MASK
    x ^= x >> 33
    return x


def subspace_seed(seed: int, m: int) -> int:
    """The seed polysemous training hands to polysemous_optimize_codebook for subspace m."""
    return mix64(seed + 0x9E3779B97F4A7C15 * (m + 1))


def optimize_codebook(codebook: np.ndarray, iters: int = 0, seed: int = 1) -> Tuple[np.ndarray, float, float]:
    """polysemous_optimize_codebook over one subspace's codewords [256, dsub]: (perm uint8 [256] -- the new number of old
    codeword j --, cost_before, cost_after).  Host only."""
    cb = np.ascontiguousarray(codebook, np.float32)
    if cb.ndim != 2 or cb.shape[0] != KSUB:
        raise ValueError(f"expected a codebook of shape [{KSUB}, dsub], got {cb.shape}")
    perm = np.empty(KSUB, np.uint8)
    before, after = C.c_double(), C.c_double()
    lib = _lib()
    _check(lib, lib.polysemous_optimize_codebook(cb.shape[1], cb.ctypes.data, iters, seed, perm.ctypes.data, C.byref(before),
                                                 C.byref(after)), lib.polysemous_last_error)
    return perm, before.value, after.value


def renumber(codebooks: np.ndarray, perms: np.ndarray) -> np.ndarray:
    """new[m][perms[m][j]] = old[m][j]: what polysemous training does to the codebooks [M, 256, dsub]."""
    cb = np.asarray(codebooks)
    out = np.empty_like(cb)
    for m in range(cb.shape[0]):
        out[m, np.asarray(perms[m], np.int64)] = cb[m]
    return out


def search_ht(index, queries: np.ndarray, k: int, nprobe: int, ht: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """ivfpq_search_ht / opq_search_ht over the handle of a FaissIvfPq / FaissOpqIvfPq or of its Polysemous twin; the handle
    stays with its holder."""
    if getattr(index, "FAISS_KIND", None) not in _TWINS:
        raise TypeError(f"{type(index).__name__} has no product-quantiser codes to filter by")
    lib = _lib()
    q = _rows(queries, getattr(index, index._row_dim))
    ids, dist, cnt = _binding.result_triple(q.shape[0], k)
    fn = getattr(lib, index._prefix + "_search_ht")
    _check(lib, fn(index._h, q.shape[0], q.ctypes.data, k, nprobe, int(ht), dist.ctypes.data, ids.ctypes.data, cnt.ctypes.data),
           getattr(lib, index._prefix + "_last_error"))
    return ids, dist, cnt


class _HtSearch:
    """search(queries, k, nprobe, ht) and the exports of the last filtered search, over the handle of either index type
    (the symbol prefix is the index class's own)."""

    def _last_error(self, lib):
        return getattr(lib, self._prefix + "_last_error")

    def search(self, queries: np.ndarray, k: int, nprobe: int, ht: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(ids [nq, k], distances [nq, k], counts [nq]) of the rows whose code is at Hamming distance < ht from the query
        code of their (query, cell) pair; ht <= 0: the unfiltered search."""
        return search_ht(self, queries, k, nprobe, ht)

    def last_query_codes(self) -> np.ndarray:
        """The query codes of the last search with ht > 0, in the order of last_probes(): uint8 [nq, nprobe, M]."""
        lib = _lib()
        fn = getattr(lib, self._prefix + "_last_query_codes")
        nq, npr = C.c_int32(), C.c_int32()
        _check(lib, fn(self._h, C.byref(nq), C.byref(npr), None), self._last_error(lib))
        out = np.empty((nq.value, npr.value, self.M), np.uint8)
        _check(lib, fn(self._h, None, None, out.ctypes.data), self._last_error(lib))
        return out

    def last_ht_stats(self) -> dict:
        lib = _lib()
        rows = C.c_int64()
        _check(lib, getattr(lib, self._prefix + "_last_ht_stats")(self._h, C.byref(rows)), self._last_error(lib))
        return {"rows_scored": rows.value}

    @property
    def is_polysemous(self) -> bool:
        """True for an index trained polysemous in this process; a loaded index does not carry the flag."""
        lib = _lib()
        out = C.c_int32()
        _check(lib, getattr(lib, self._prefix + "_index_is_polysemous")(self._h, C.byref(out)), self._last_error(lib))
        return bool(out.value)


class PolysemousIvfPq(_HtSearch, FaissIvfPq):
    """FaissIvfPq with polysemous training and the filtered search."""

    @classmethod
    def train(cls, metric: DistanceMetric, nlist: int, M: int, train_vectors: np.ndarray, *, niter: int = 0, seed: int = 1,
              anneal_iters: int = 0, device: int = 0):
        """FaissIvfPq.train, then the codewords of every subspace renumbered (anneal_iters: 0 = 500,000 steps each)."""
        lib = _lib()
        v = _rows(train_vectors)
        h = C.c_void_p()
        _check(lib, lib.ivfpq_index_train_polysemous(device, int(metric), v.shape[1], nlist, M, v.shape[0], v.ctypes.data, niter,
                                                     seed, anneal_iters, C.byref(h)), lib.ivfpq_last_error)
        return cls(h, metric, v.shape[1], nlist, M)

    @classmethod
    def adopt(cls, index: FaissIvfPq):
        """Takes over the handle of a FaissIvfPq (one that faiss_files loaded, say); `index` is closed to its holder."""
        out = cls(None, index.metric, index.d, index.nlist, index.M)
        out._take(index)
        return out


class PolysemousOpqIvfPq(_HtSearch, FaissOpqIvfPq):
    """FaissOpqIvfPq with polysemous training of the inner index and the filtered search."""

    @classmethod
    def train(cls, metric: DistanceMetric, nlist: int, M: int, d_out: int, train_vectors: np.ndarray, *, niter: int = 0,
              niter_opq: int = 0, seed: int = 1, anneal_iters: int = 0, device: int = 0):
        lib = _lib()
        v = _rows(train_vectors)
        h = C.c_void_p()
        _check(lib, lib.opq_index_train_polysemous(device, int(metric), v.shape[1], d_out, nlist, M, v.shape[0], v.ctypes.data, niter,
                                                   niter_opq, seed, anneal_iters, C.byref(h)), lib.opq_last_error)
        return cls(h, metric, v.shape[1], d_out, nlist, M)

    @classmethod
    def adopt(cls, index: FaissOpqIvfPq):
        out = cls(None, index.metric, index.d_in, index.d_out, index.nlist, index.M)
        out._take(index)
        return out


_TWINS = {FaissIvfPq.FAISS_KIND: PolysemousIvfPq, FaissOpqIvfPq.FAISS_KIND: PolysemousOpqIvfPq}


def adopt(index):
    """The Polysemous* twin of a FaissIvfPq / FaissOpqIvfPq, over the same handle."""
    if isinstance(index, _HtSearch):
        return index
    twin = _TWINS.get(getattr(index, "FAISS_KIND", None))
    if twin is None:
        raise TypeError(f"{type(index).__name__} has no product-quantiser codes to filter by")
    return twin.adopt(index)


_FACTORY = re.compile(r"(?:OPQ(\d+)(?:_(\d+))?,)?IVF(\d+),PQ(\d+)(?:x8)?(np)?")


class PolysemousIndexSpec:
    """What index_factory returns: an untrained index.  train() yields the trained, empty Polysemous(Opq)IvfPq --
    polysemous unless the string ends in `np`."""

    def __init__(self, dimension: int, metric: DistanceMetric, d_out: Optional[int], nlist: int, M: int, polysemous: bool,
                 factory_string: str):
        self.dimension, self.metric, self.d_out, self.nlist, self.M = dimension, DistanceMetric(metric), d_out, nlist, M
        self.polysemous, self.factory_string = polysemous, factory_string

    @property
    def index_class(self):
        return PolysemousIvfPq if self.d_out is None else PolysemousOpqIvfPq

    def train(self, vectors: np.ndarray, niter: int = 0, seed: int = 1, *, niter_opq: int = 0, anneal_iters: int = 0, device: int = 0):
        v = _rows(vectors, self.dimension)
        if self.d_out is None:
            if self.polysemous:
                return PolysemousIvfPq.train(self.metric, self.nlist, self.M, v, niter=niter, seed=seed, anneal_iters=anneal_iters,
                                             device=device)
            return PolysemousIvfPq.adopt(FaissIvfPq.train(self.metric, self.nlist, self.M, v, niter=niter, seed=seed, device=device))
        if self.polysemous:
            return PolysemousOpqIvfPq.train(self.metric, self.nlist, self.M, self.d_out, v, niter=niter, niter_opq=niter_opq, seed=seed,
                                            anneal_iters=anneal_iters, device=device)
        return PolysemousOpqIvfPq.adopt(FaissOpqIvfPq.train(self.metric, self.nlist, self.M, self.d_out, v, niter=niter,
                                                            niter_opq=niter_opq, seed=seed, device=device))


def index_factory(dimension: int, factory_string: str, metric: DistanceMetric) -> PolysemousIndexSpec:
    """Faiss's index_factory for `IVF<nlist>,PQ<M>[x8]` and `OPQ<M>[_<dout>],IVF<nlist>,PQ<M>[x8]`, which it trains
    polysemous, and for the same strings with `np` appended, which it trains plain.  The shapes are checked by the older
    factories (opq_ann.index_factory, ivfpq_ann.index_factory), whose refusals are this one's."""
    m = _FACTORY.fullmatch(factory_string) if isinstance(factory_string, str) else None
    if m is None:
        raise ValueError(f"index_factory: unsupported factory string {factory_string!r} (IVF<nlist>,PQ<M>[x8][np] and "
                         "OPQ<M>[_<dout>],IVF<nlist>,PQ<M>[x8][np] are served)")
    plain = factory_string[:-2] if m.group(5) else factory_string
    spec = opq_ann.index_factory(dimension, plain, metric)
    d_out = spec.d_out if isinstance(spec, opq_ann.OpqIndexSpec) else None
    return PolysemousIndexSpec(int(dimension), metric, d_out, spec.nlist, spec.M, m.group(5) is None, factory_string)


def build_faiss_index(vectors: np.ndarray, ids: Sequence[int], sample_rate: float, factory_string: Optional[str] = None,
                      metric: DistanceMetric = DistanceMetric.Cosine, *, niter: int = 0, niter_opq: int = 0, seed: int = 1,
                      anneal_iters: int = 0, device: int = 0):
    """opq_ann.build_faiss_index over this module's index_factory: the default factory string of
    faiss_index_bq_dataset.py, and any other served string, builds what Faiss builds from it -- a polysemous index."""
    v = _rows(vectors)
    if factory_string is None:
        factory_string = opq_ann.default_factory_string(v.shape[0], v.shape[1])
    spec = index_factory(v.shape[1], factory_string, metric)
    head = v[:ivfpq_ann.training_set_size(v.shape[0], sample_rate)]
    index = spec.train(head, niter, seed, niter_opq=niter_opq, anneal_iters=anneal_iters, device=device)
    index.add(v, ids)
    return index


class PolysemousFaissQueryable(FaissQueryable):
    """FaissQueryable over a Polysemous(Opq)IvfPq: FaissParams.nprobe and FaissParams.ht are served (ht unset or <= 0: no
    filter, as in Faiss); the three quantizer* fields stay refused -- the coarse search here is exact."""

    def __init__(self, index, metric: DistanceMetric):
        # (anything else with search(queries, k, nprobe, ht) is served as it is, as FaissQueryable serves any search())
        super().__init__(adopt(index) if isinstance(index, (FaissIvfPq, FaissOpqIvfPq)) else index, metric)

    @staticmethod
    def _params(params: FaissParams) -> Tuple[int, int]:
        others = [f for f in ("quantizerEf", "quantizerKfactorRf", "quantizerNprobe") if getattr(params, f) is not None]
        if others:
            raise ValueError("the coarse quantizer of this index is an exact search, with no HNSW graph, refinement or inner "
                             "nprobe to tune: " + ", ".join(others) + " cannot be set (only nprobe and ht)")
        if params.nprobe is None:
            raise ValueError("FaissParams.nprobe must be set")
        return int(params.nprobe), 0 if params.ht is None else int(params.ht)

    def queryWithDistance(self, embedding: np.ndarray, numOfNeighbors: int, runtimeParams: FaissParams) -> List[Tuple[int, float]]:
        nprobe, ht = self._params(runtimeParams)
        ids, dist, cnt = self.index.search(np.asarray(embedding, np.float32), numOfNeighbors, nprobe, ht)
        m = int(cnt[0])
        out_d = np.array(dist[0, :m], np.float32)
        if self.metric == DistanceMetric.Cosine:
            sim = np.float32(1.0) - out_d
            out_d = np.where((sim < 0) | (sim > 1), np.float32(MAX_COSINE_DISTANCE), out_d).astype(np.float32)
        return list(zip(np.asarray(ids[0, :m]).tolist(), out_d.tolist()))
