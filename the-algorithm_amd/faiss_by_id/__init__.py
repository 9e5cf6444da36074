"""ctypes binding of include/faiss_by_id.h and the reference's QueryableById over the inverted-file family and shard sets.

Reference (paths relative to the reference's ann/src/main/scala/com/twitter/ann/common/):
  Api.scala                                  trait QueryableById: queryById, queryByIdWithDistance, batchQueryById,
                                             batchQueryWithDistanceById
  QueryableByIdImplementation.scala:15-91    the composition of an EmbeddingProducer with a Queryable
The producer is ann_by_id.EmbeddingStore, resident on the device beside the index: a call uploads the seed ids and downloads
the flattened triples; the rows are read out of the store by the index's own query preparation.  The answer of a found seed is,
byte for byte, the plain search over EmbeddingStore.get(seed).

Imported by name (`the_algorithm_amd.faiss_by_id`); the package does not re-export it.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .. import binding as _binding
from .. import hnsw_quantizer
from ..ann_by_id import EmbeddingStore, _keys
from ..dense_ann import DistanceMetric
from ..faiss_files import HourlyShardedIndex
from ..ivf_ann import FaissIvfFlat, FaissParams, FaissQueryable, IvfError
from ..ivfpq_ann import FaissIvfPq
from ..opq_ann import FaissOpqIvfPq
from ..scalar_quantizer import FaissIvfSq8
from ..shard_set import ShardSet
from ..simclusters_ann import load_library

_P = C.POINTER
_HEAD = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]           # index, store, n_seeds, seeds, k, nprobe
_TAIL = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, _P(C.c_int64), C.c_void_p]       # out_seed, out_id, out_dist, cap, out_total, out_counts
PROTOS = {
    "ivf_by_id_last_error": (C.c_char_p, []),
    "ivf_batch_query_by_id": (C.c_int, _HEAD + _TAIL),
    "ivfsq_batch_query_by_id": (C.c_int, _HEAD + _TAIL),
    "ivfpq_batch_query_by_id": (C.c_int, _HEAD + [C.c_int32] + _TAIL),
    "opq_batch_query_by_id": (C.c_int, _HEAD + [C.c_int32] + _TAIL),
    "shard_set_batch_query_by_id": (C.c_int, _HEAD + [C.c_int32] + _TAIL),
    "ivf_by_id_last_stats": (C.c_int, [C.c_int32, C.c_void_p] + [_P(C.c_int64)] * 5 + [_P(C.c_float)] * 3),
}

# FAISS_BY_ID_* of the header
KIND_IVF_FLAT, KIND_IVF_PQ, KIND_OPQ_IVF_PQ, KIND_IVF_SQ8, KIND_SHARD_SET = 1, 2, 3, 4, 5


class FaissByIdError(IvfError):
    """A status other than 0 from faiss_by_id.h; `code` is the status (1 = EINVAL, 3 = ELIMIT)."""

    def __init__(self, code: int, message: str):
        super().__init__(f"faiss_by_id error {code}: {message}")
        self.code, self.message = code, message


_lib = _binding.binder(PROTOS, "faiss_by_id", load_library)
_check = _binding.checker(FaissByIdError, "faiss_by_id", "ivf_by_id_last_error", with_code=True)

# (class, symbol prefix, FAISS_BY_ID_*, takes ht, the attribute that holds the dimension of incoming rows); subclasses
# (the polysemous twins) match their base
_KINDS = ((FaissIvfFlat, "ivf", KIND_IVF_FLAT, False, "d"), (FaissIvfSq8, "ivfsq", KIND_IVF_SQ8, False, "d"),
          (FaissIvfPq, "ivfpq", KIND_IVF_PQ, True, "d"), (FaissOpqIvfPq, "opq", KIND_OPQ_IVF_PQ, True, "d_in"),
          (ShardSet, "shard_set", KIND_SHARD_SET, True, "dimension"))


class _Row:
    """One answered row in the place of an index: FaissQueryable.queryWithDistance reads it through search() and translates
    its distances, so the translation is that code, not a copy of it."""

    def __init__(self, ids: np.ndarray, dist: np.ndarray):
        self._ids, self._dist = ids, dist

    def search(self, queries, k, nprobe):
        return self._ids[None, :], self._dist[None, :], np.array([self._ids.shape[0]], np.int32)


class FaissQueryableById:
    """QueryableByIdImplementation over an EmbeddingStore and a FaissIvfFlat, FaissIvfSq8, FaissIvfPq, FaissOpqIvfPq (or a
    polysemous twin), ShardSet or HourlyShardedIndex.  runtimeParams is a FaissParams: nprobe is required; ht goes to an
    index with product-quantiser codes (and to a set, which refuses it when it has an IVF-Flat member) and is refused by
    name elsewhere; quantizerEf is set on an index that carries an HNSW quantizer and refused otherwise; quantizerKfactorRf
    and quantizerNprobe are refused, as everywhere.  Distances are translated as FaissQueryable translates them."""

    def __init__(self, store: EmbeddingStore, index, metric: DistanceMetric):
        if not isinstance(store, EmbeddingStore):
            raise TypeError("store must be an EmbeddingStore: these indexes keep no fp32 rows of their own")
        for cls, prefix, kind, has_ht, dim in _KINDS:
            if isinstance(index, cls):
                break
        else:
            if not isinstance(index, HourlyShardedIndex):
                raise TypeError("index must be a FaissIvfFlat, FaissIvfSq8, FaissIvfPq, FaissOpqIvfPq, ShardSet or HourlyShardedIndex")
            prefix, kind, has_ht, dim = "shard_set", KIND_SHARD_SET, True, "dimension"
        if store.d != getattr(index, dim):
            raise ValueError(f"store dimension {store.d} != index {dim} {getattr(index, dim)}")
        self.store, self.index, self.metric = store, index, DistanceMetric(metric)
        self._prefix, self._kind, self._has_ht = prefix, kind, has_ht
        self._translate = FaissQueryable(None, self.metric)

    def _handle(self):
        if isinstance(self.index, HourlyShardedIndex):
            if self.index._set is None:
                raise RuntimeError("no shard was ever loaded: call reload() first")
            return self.index._set._h
        return self.index._h

    def _params(self, params) -> Tuple[int, int, Optional[int]]:
        """(nprobe, ht, quantizer_ef or None) of a FaissParams, refusing by name what this index cannot take."""
        if not isinstance(params, FaissParams):
            raise TypeError("runtimeParams must be a FaissParams(nprobe=...)")
        others = [f for f in ("quantizerKfactorRf", "quantizerNprobe") if getattr(params, f) is not None]
        if others:
            raise ValueError("no index here has a refinement factor or an inner nprobe to tune: " + ", ".join(others) + " cannot be set")
        if params.ht is not None and not self._has_ht:
            raise ValueError(f"{type(self.index).__name__} has no product-quantiser codes to filter by: ht cannot be set")
        if params.nprobe is None:
            raise ValueError("FaissParams.nprobe must be set")
        ef = None
        if params.quantizerEf is not None:
            if self._kind in (KIND_IVF_SQ8, KIND_SHARD_SET) or not hnsw_quantizer.info(self.index)["attached"]:
                raise ValueError(f"this {type(self.index).__name__} carries no HNSW quantizer: quantizerEf cannot be set")
            ef = int(params.quantizerEf)
        return int(params.nprobe), 0 if params.ht is None else int(params.ht), ef

    def batch_arrays(self, ids: Sequence[int], numOfNeighbors: int, runtimeParams: FaissParams, cap: Optional[int] = None):
        """The library call as arrays: (seeds [total], neighbours [total], distances [total], counts [n_seeds]; -1 = absent).
        The distances are the index's own (untranslated)."""
        seeds = _keys(ids, "ids")
        k = int(numOfNeighbors)
        if k < 1:
            raise ValueError("numOfNeighbors must be positive")
        nprobe, ht, ef = self._params(runtimeParams)
        n = seeds.shape[0]
        cap = n * k if cap is None else int(cap)
        o_seed = np.zeros(max(cap, 1), np.int64); o_id = np.zeros(max(cap, 1), np.int64); o_dist = np.zeros(max(cap, 1), np.float32)
        counts = np.zeros(max(n, 1), np.int32)
        total = C.c_int64()
        lib = _lib()
        if ef is not None:
            hnsw_quantizer.set_quantizer_ef(self.index, ef)
        head = (self._handle(), self.store._h, n, seeds.ctypes.data, k, nprobe) + ((ht,) if self._has_ht else ())
        _check(lib, getattr(lib, self._prefix + "_batch_query_by_id")(*head, o_seed.ctypes.data, o_id.ctypes.data, o_dist.ctypes.data, cap,
                                                                      C.byref(total), counts.ctypes.data))
        t = total.value
        return o_seed[:t], o_id[:t], o_dist[:t], counts[:n]

    def _translated(self, ids, numOfNeighbors, runtimeParams):
        s, i, d, c = self.batch_arrays(ids, numOfNeighbors, runtimeParams)
        out_d, at = np.array(d, np.float32), 0
        for m in c.tolist():
            if m > 0:
                self._translate.index = _Row(i[at:at + m], d[at:at + m])
                out_d[at:at + m] = [x for _, x in self._translate.queryWithDistance(np.zeros(1, np.float32), m, FaissParams(nprobe=1))]
                at += m
        self._translate.index = None
        return s, i, out_d

    def batchQueryWithDistanceById(self, ids: Sequence[int], numOfNeighbors: int, runtimeParams: FaissParams) -> List[Tuple[int, int, float]]:
        """NeighborWithDistanceWithSeed(seed, neighbor, distance) in seed order (QueryableByIdImplementation.scala:69-90)."""
        s, i, d = self._translated(ids, numOfNeighbors, runtimeParams)
        return list(zip(s.tolist(), i.tolist(), d.tolist()))

    def batchQueryById(self, ids: Sequence[int], numOfNeighbors: int, runtimeParams: FaissParams) -> List[Tuple[int, int]]:
        """NeighborWithSeed(seed, neighbor) in seed order (:48-67)."""
        s, i, _, _ = self.batch_arrays(ids, numOfNeighbors, runtimeParams)
        return list(zip(s.tolist(), i.tolist()))

    def queryByIdWithDistance(self, id: int, numOfNeighbors: int, runtimeParams: FaissParams) -> List[Tuple[int, float]]:
        """NeighborWithDistance of one id; an absent id gives nothing (:32-46)."""
        _, i, d = self._translated([id], numOfNeighbors, runtimeParams)
        return list(zip(i.tolist(), d.tolist()))

    def queryById(self, id: int, numOfNeighbors: int, runtimeParams: FaissParams) -> List[int]:
        """(:19-30)."""
        return [i for i, _ in self.queryByIdWithDistance(id, numOfNeighbors, runtimeParams)]

    def last_stats(self) -> dict:
        """Figures of the last call on this index: seeds found / absent, bus bytes, HIP-event times of the three phases."""
        v = [C.c_int64() for _ in range(5)]
        f = [C.c_float() for _ in range(3)]
        lib = _lib()
        _check(lib, lib.ivf_by_id_last_stats(self._kind, self._handle(), *[C.byref(x) for x in v], *[C.byref(x) for x in f]))
        names = ("found", "absent", "h2d_bytes", "d2h_bytes", "d2h_result_bytes", "resolve_gather_ms", "search_ms", "flatten_ms")
        return dict(zip(names, [x.value for x in v] + [x.value for x in f]))
