"""ctypes binding of include/ann_by_id.h and a host-side mirror of the reference's QueryableById.

Reference (paths relative to /root/reference/ann/src/main/scala/com/twitter/ann/common/):
  EmbeddingProducer.scala                    produceEmbedding(id): Option[embedding]
  Api.scala                                  trait QueryableById: queryById, queryByIdWithDistance, batchQueryById,
                                             batchQueryWithDistanceById
  QueryableByIdImplementation.scala:15-91    the composition of an EmbeddingProducer with a Queryable
The embeddings live on the device beside the index: a call uploads the seed ids and downloads the flattened triples.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from . import binding as _binding
from .dense_ann import BruteForceIndex
from .hnsw_ann import Hnsw, HnswParams
from .simclusters_ann import load_library

PROTOS = {
    "ann_by_id_last_error": (C.c_char_p, []),
    "ann_store_build": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "ann_store_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "ann_store_get": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ann_store_destroy": (C.c_int, [C.c_void_p]),
    "hnsw_batch_query_by_id": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
    "dann_batch_query_by_id": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
    "ann_by_id_last_stats": (C.c_int, [C.c_void_p, C.c_void_p] + [C.POINTER(C.c_int64)] * 5 + [C.POINTER(C.c_float)] * 3),
}


class AnnByIdError(RuntimeError):
    pass


_lib = _binding.binder(PROTOS, "ann_by_id", load_library)
_check = _binding.checker(AnnByIdError, "ann_by_id", "ann_by_id_last_error")


def _keys(keys, what: str) -> np.ndarray:
    a = np.asarray(keys)
    if a.ndim != 1:
        raise ValueError(f"{what} must be one-dimensional, got shape {a.shape}")
    if a.size and a.dtype.kind not in "iu":
        raise ValueError(f"{what} must be integers, got dtype {a.dtype}")
    return np.ascontiguousarray(a, np.int64)


class EmbeddingStore(_binding.Handle):
    """EmbeddingProducer resident in HBM: fp32 rows under unique int64 keys (ann_store_build).  Immutable once built."""

    _destroy, _lib = "ann_store_destroy", staticmethod(_lib)

    def __init__(self, handle, n: int, d: int):
        self._h, self.n, self.d = handle, n, d

    @classmethod
    def build(cls, keys: Sequence[int], vectors: np.ndarray, device: int = 0) -> "EmbeddingStore":
        k = _keys(keys, "keys")
        v = np.asarray(vectors)
        if v.ndim != 2:
            raise ValueError(f"vectors must be [n][d], got shape {v.shape}")
        if v.dtype.kind != "f":
            raise ValueError(f"vectors must be floating point, got dtype {v.dtype}")
        if k.shape[0] != v.shape[0]:
            raise ValueError(f"one key per vector: {k.shape[0]} keys, {v.shape[0]} vectors")
        v = np.ascontiguousarray(v, np.float32)
        lib = _lib()
        h = C.c_void_p()
        _check(lib, lib.ann_store_build(device, v.shape[0], v.shape[1], k.ctypes.data, v.ctypes.data, C.byref(h)))
        return cls(h, v.shape[0], v.shape[1])

    def get(self, keys: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
        """produceEmbedding for every key: (rows [n][d] fp32, found [n] bool); an absent key's row is zeros."""
        k = _keys(keys, "keys")
        out = np.zeros((k.shape[0], self.d), np.float32)
        found = np.zeros(k.shape[0], np.uint8)
        lib = _lib()
        _check(lib, lib.ann_store_get(self._h, k.shape[0], k.ctypes.data, out.ctypes.data, found.ctypes.data))
        return out, found.astype(bool)


class QueryableById:
    """QueryableByIdImplementation: an EmbeddingStore (None: the index's own keys and rows) composed with an Hnsw or a
    BruteForceIndex.  runtimeParams is an HnswParams for an Hnsw and ignored for a BruteForceIndex."""

    def __init__(self, store: Optional[EmbeddingStore], index: Union[Hnsw, BruteForceIndex]):
        if not isinstance(index, (Hnsw, BruteForceIndex)):
            raise TypeError("index must be an Hnsw or a BruteForceIndex")
        if store is not None and not isinstance(store, EmbeddingStore):
            raise TypeError("store must be an EmbeddingStore or None")
        if store is not None and store.d != index.d:
            raise ValueError(f"store dimension {store.d} != index dimension {index.d}")
        self.store, self.index = store, index
        self._hnsw = isinstance(index, Hnsw)

    def batch_arrays(self, ids: Sequence[int], numOfNeighbors: int, runtimeParams: Optional[HnswParams] = None, cap: Optional[int] = None):
        """The library call as arrays: (seeds [total], neighbours [total], distances [total], counts [n_seeds]; -1 = absent)."""
        seeds = _keys(ids, "ids")
        k = int(numOfNeighbors)
        if k < 1:
            raise ValueError("numOfNeighbors must be positive")
        if self._hnsw and not isinstance(runtimeParams, HnswParams):
            raise TypeError("an Hnsw index needs runtimeParams = HnswParams(ef)")
        n = seeds.shape[0]
        cap = n * k if cap is None else int(cap)
        o_seed = np.zeros(max(cap, 1), np.int64); o_id = np.zeros(max(cap, 1), np.int64); o_dist = np.zeros(max(cap, 1), np.float32)
        counts = np.zeros(max(n, 1), np.int32)
        total = C.c_int64()
        lib = _lib()
        sh = self.store._h if self.store is not None else None
        if self._hnsw:
            rc = lib.hnsw_batch_query_by_id(self.index._h, sh, n, seeds.ctypes.data, k, int(runtimeParams.ef), o_seed.ctypes.data,
                                            o_id.ctypes.data, o_dist.ctypes.data, cap, C.byref(total), counts.ctypes.data)
        else:
            rc = lib.dann_batch_query_by_id(self.index._h, sh, n, seeds.ctypes.data, k, o_seed.ctypes.data, o_id.ctypes.data,
                                            o_dist.ctypes.data, cap, C.byref(total), counts.ctypes.data)
        _check(lib, rc)
        t = total.value
        return o_seed[:t], o_id[:t], o_dist[:t], counts[:n]

    def batchQueryWithDistanceById(self, ids: Sequence[int], numOfNeighbors: int, runtimeParams: Optional[HnswParams] = None
                                   ) -> List[Tuple[int, int, float]]:
        """NeighborWithDistanceWithSeed(seed, neighbor, distance) in seed order (QueryableByIdImplementation.scala:69-90)."""
        s, i, d, _ = self.batch_arrays(ids, numOfNeighbors, runtimeParams)
        return list(zip(s.tolist(), i.tolist(), d.tolist()))

    def batchQueryById(self, ids: Sequence[int], numOfNeighbors: int, runtimeParams: Optional[HnswParams] = None) -> List[Tuple[int, int]]:
        """NeighborWithSeed(seed, neighbor) in seed order (:48-67)."""
        s, i, _, _ = self.batch_arrays(ids, numOfNeighbors, runtimeParams)
        return list(zip(s.tolist(), i.tolist()))

    def queryByIdWithDistance(self, id: int, numOfNeighbors: int, runtimeParams: Optional[HnswParams] = None) -> List[Tuple[int, float]]:
        """NeighborWithDistance of one id; an absent id gives nothing (:32-46)."""
        _, i, d, _ = self.batch_arrays([id], numOfNeighbors, runtimeParams)
        return list(zip(i.tolist(), d.tolist()))

    def queryById(self, id: int, numOfNeighbors: int, runtimeParams: Optional[HnswParams] = None) -> List[int]:
        """(:19-30)."""
        return [i for i, _ in self.queryByIdWithDistance(id, numOfNeighbors, runtimeParams)]

    def last_stats(self) -> dict:
        """Figures of the last call on this index: seeds found / absent, bus bytes, HIP-event times of the three phases."""
        v = [C.c_int64() for _ in range(5)]
        f = [C.c_float() for _ in range(3)]
        lib = _lib()
        h, dn = (self.index._h, None) if self._hnsw else (None, self.index._h)
        _check(lib, lib.ann_by_id_last_stats(h, dn, *[C.byref(x) for x in v], *[C.byref(x) for x in f]))
        names = ("found", "absent", "h2d_bytes", "d2h_bytes", "d2h_result_bytes", "resolve_gather_ms", "search_ms", "flatten_ms")
        return dict(zip(names, [x.value for x in v] + [x.value for x in f]))
