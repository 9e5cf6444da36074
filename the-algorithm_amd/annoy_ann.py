"""ctypes binding of include/annoy_ann.h: the Annoy index -- a forest of random-projection trees built on the host, a
best-first walk and an exact re-score on the device.

Reference (paths relative to the reference's ann/src/main/):
  scala/com/twitter/ann/annoy/RawAnnoyIndexBuilder.scala:53-65    append: the counter 1, 2, ... is the id; toQueryable
  scala/com/twitter/ann/annoy/RawAnnoyQueryIndex.scala:48-54      L2 and Cosine; InnerProduct "Not supported"
  scala/com/twitter/ann/annoy/RawAnnoyQueryIndex.scala:124-138    neighboursToRequest
  scala/com/twitter/ann/annoy/TypedAnnoyIndex.scala               caller ids over the counter
  thrift/com/twitter/ann/common/ann_common.thrift:129-133         RuntimeParams case 1: annoyParam
Not here: building on the device, Annoy's file format, JNI, by-id queries, membership in a ShardSet.  The phantom all-zero
item 0 of the reference's library (its counter starts at 1) is not reproduced.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import binding as _binding
from .dense_ann import DistanceMetric
from .ivf_ann import IvfError, _rows
from .simclusters_ann import load_library

_P = C.POINTER
PROTOS = {
    "annoy_last_error": (C.c_char_p, []),
    "annoy_prepare_rows": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    "annoy_forest_build": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_int32,
                                     _P(C.c_void_p)]),
    "annoy_forest_load": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int64,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, _P(C.c_void_p)]),
    "annoy_forest_info": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), _P(C.c_int64), _P(C.c_int32), _P(C.c_int32),
                                    _P(C.c_int64), _P(C.c_int64), _P(C.c_int64)]),
    "annoy_forest_get_nodes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "annoy_forest_get_normals": (C.c_int, [C.c_void_p, C.c_void_p]),
    "annoy_forest_get_offsets": (C.c_int, [C.c_void_p, C.c_void_p]),
    "annoy_forest_get_roots": (C.c_int, [C.c_void_p, C.c_void_p]),
    "annoy_forest_get_items": (C.c_int, [C.c_void_p, C.c_void_p]),
    "annoy_forest_destroy": (C.c_int, [C.c_void_p]),
    "annoy_index_from_forest": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, _P(C.c_void_p)]),
    "annoy_index_build": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                    C.c_uint64, C.c_int32, _P(C.c_void_p)]),
    "annoy_search": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "annoy_index_info": (C.c_int, [C.c_void_p, _P(C.c_int64), _P(C.c_int32), _P(C.c_int32), _P(C.c_int32), _P(C.c_int32),
                                   _P(C.c_int64)]),
    "annoy_index_get_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "annoy_index_forest": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "annoy_last_candidates": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), C.c_void_p, C.c_void_p]),
    "annoy_last_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, _P(C.c_int32), _P(C.c_int32), _P(C.c_float), _P(C.c_float),
                                   _P(C.c_float)]),
    "annoy_debug_set_limits": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64]),
    "annoy_index_destroy": (C.c_int, [C.c_void_p]),
}

MAX_D, MAX_TREES, MAX_LEAF, MAX_K, MAX_SEARCH_K = 1024, 1024, 2048, 1024, 262144
NODE_SPLIT, NODE_LEAF, NODE_FALLBACK = 0, 1, 1


class AnnoyError(IvfError):
    pass


_lib = _binding.binder(PROTOS, "annoy", load_library)
_check = _binding.checker(AnnoyError, "annoy_ann", "annoy_last_error")


def _metric(metric) -> DistanceMetric:
    metric = DistanceMetric(metric)
    if metric not in (DistanceMetric.L2, DistanceMetric.Cosine):
        raise ValueError(f"Not supported: {metric.name} (an Annoy index is L2 or Cosine)")  # RawAnnoyQueryIndex.scala:52
    return metric


@dataclasses.dataclass(frozen=True)
class AnnoyRuntimeParams:
    """ann_common.thrift: AnnoyRuntimeParam {1: optional i32 numOfNodesToExplore}."""

    nodesToExplore: Optional[int] = None


def neighbours_to_request(k: int, params: AnnoyRuntimeParams, n_trees: int) -> int:
    """RawAnnoyQueryIndex.scala:124-138: nodesToExplore / numOfTrees (integer division) where that is at least k, else k."""
    if params is None or params.nodesToExplore is None:
        return k
    return max(k, int(params.nodesToExplore) // n_trees)


def prepare(metric, rows: np.ndarray) -> np.ndarray:
    """Rows as the index stores them (and a query as the walk sees it): float16 [n, d]."""
    v = _rows(rows)
    out = np.empty(v.shape, np.float16)
    lib = _lib()
    _check(lib, lib.annoy_prepare_rows(int(metric), v.shape[1], v.shape[0], v.ctypes.data, out.ctypes.data))
    return out


class AnnoyForest(_binding.Handle):
    """The forest in its flat host form: build() it from rows or load() it from arrays; the arrays are properties.  Host
    only: no device is touched."""

    _destroy, _lib = "annoy_forest_destroy", staticmethod(_lib)

    def __init__(self, handle, owned: bool = True, keeper=None):
        self._h, self._owned, self._keeper = handle, owned, keeper

    @classmethod
    def build(cls, metric, rows: np.ndarray, n_trees: int, leaf_size: int = 0, seed: int = 1, threads: int = 0):
        lib = _lib()
        v = _rows(rows)
        h = C.c_void_p()
        _check(lib, lib.annoy_forest_build(int(metric), v.shape[1], v.shape[0], v.ctypes.data, n_trees, leaf_size, seed, threads,
                                           C.byref(h)))
        return cls(h)

    @classmethod
    def load(cls, metric, d: int, n: int, leaf_size: int, nodes, normals, offsets, roots, items):
        lib = _lib()
        nodes = np.ascontiguousarray(nodes, np.int32).reshape(-1, 4)
        offsets = np.ascontiguousarray(offsets, np.float32).reshape(-1)
        normals = np.ascontiguousarray(normals)
        if normals.dtype != np.uint16:
            normals = normals.astype(np.float16).view(np.uint16)
        normals = np.ascontiguousarray(normals).reshape(-1, d)
        if len(normals) != len(offsets):
            raise ValueError("one offset per normal")
        roots = np.ascontiguousarray(roots, np.int32).reshape(-1)
        items = np.ascontiguousarray(items, np.int32).reshape(-1)
        h = C.c_void_p()
        _check(lib, lib.annoy_forest_load(int(metric), d, n, len(roots), leaf_size, len(nodes), nodes.ctypes.data, len(offsets),
                                          normals.ctypes.data, offsets.ctypes.data, roots.ctypes.data, len(items), items.ctypes.data,
                                          C.byref(h)))
        return cls(h)

    def info(self) -> dict:
        metric, d, nt, leaf = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        n, nn, ns, ni = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        lib = _lib()
        _check(lib, lib.annoy_forest_info(self._h, C.byref(metric), C.byref(d), C.byref(n), C.byref(nt), C.byref(leaf), C.byref(nn),
                                          C.byref(ns), C.byref(ni)))
        return {"metric": DistanceMetric(metric.value), "d": d.value, "n": n.value, "n_trees": nt.value, "leaf_size": leaf.value,
                "n_nodes": nn.value, "n_splits": ns.value, "n_items": ni.value}

    def _get(self, fn, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype)
        lib = _lib()
        _check(lib, getattr(lib, fn)(self._h, out.ctypes.data))
        return out

    @property
    def nodes(self) -> np.ndarray:
        """int32 [n_nodes, 4]: kind, a, b, flags."""
        return self._get("annoy_forest_get_nodes", (self.info()["n_nodes"], 4), np.int32)

    @property
    def normals(self) -> np.ndarray:
        """float16 [n_splits, d], in the node order of the splits."""
        i = self.info()
        return self._get("annoy_forest_get_normals", (i["n_splits"], i["d"]), np.float16)

    @property
    def offsets(self) -> np.ndarray:
        return self._get("annoy_forest_get_offsets", (self.info()["n_splits"],), np.float32)

    @property
    def roots(self) -> np.ndarray:
        return self._get("annoy_forest_get_roots", (self.info()["n_trees"],), np.int32)

    @property
    def items(self) -> np.ndarray:
        return self._get("annoy_forest_get_items", (self.info()["n_items"],), np.int32)


class AnnoyQueryable(_binding.Handle):
    """The Annoy index resident in HBM, immutable: from_forest() or build(), then query / queryWithDistance / search."""

    _destroy, _lib = "annoy_index_destroy", staticmethod(_lib)

    def __init__(self, handle, metric: DistanceMetric, d: int, n_trees: int):
        self._h, self.metric, self.d, self.n_trees = handle, metric, d, n_trees

    @classmethod
    def from_forest(cls, forest: AnnoyForest, rows: np.ndarray, ids: Optional[Sequence[int]] = None, device: int = 0):
        lib = _lib()
        i = forest.info()
        v = _rows(rows, i["d"])
        if v.shape[0] != i["n"]:
            raise ValueError(f"the forest was built over {i['n']} rows, got {v.shape[0]}")
        idp = _binding.ids_or_none(ids, v.shape[0], "row")
        h = C.c_void_p()
        _check(lib, lib.annoy_index_from_forest(device, forest._h, v.ctypes.data, _binding.ptr(idp),
                                                C.byref(h)))
        return cls(h, i["metric"], i["d"], i["n_trees"])

    @classmethod
    def build(cls, metric, rows: np.ndarray, n_trees: int, ids: Optional[Sequence[int]] = None, leaf_size: int = 0, seed: int = 1,
              threads: int = 0, device: int = 0):
        lib = _lib()
        metric = _metric(metric)
        v = _rows(rows)
        idp = _binding.ids_or_none(ids, v.shape[0], "row")
        h = C.c_void_p()
        _check(lib, lib.annoy_index_build(device, int(metric), v.shape[1], v.shape[0], v.ctypes.data,
                                          _binding.ptr(idp), n_trees, leaf_size, seed, threads, C.byref(h)))
        return cls(h, metric, v.shape[1], n_trees)

    def info(self) -> dict:
        n, nn = C.c_int64(), C.c_int64()
        d, metric, nt, leaf = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        lib = _lib()
        _check(lib, lib.annoy_index_info(self._h, C.byref(n), C.byref(d), C.byref(metric), C.byref(nt), C.byref(leaf), C.byref(nn)))
        return {"n": n.value, "d": d.value, "metric": DistanceMetric(metric.value), "n_trees": nt.value, "leaf_size": leaf.value,
                "n_nodes": nn.value}

    @property
    def n(self) -> int:
        return self.info()["n"]

    def search(self, queries: np.ndarray, k: int, nodes_to_explore: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(ids [nq, k], distances [nq, k], counts [nq]): ascending by (distance, id); 0 / 0 past the count."""
        lib = _lib()
        q = _rows(queries, self.d)
        nq = q.shape[0]
        ids, dist, cnt = _binding.result_triple(nq, k, clamp=True)
        _check(lib, lib.annoy_search(self._h, nq, q.ctypes.data, k, -1 if nodes_to_explore is None else int(nodes_to_explore),
                                     dist.ctypes.data, ids.ctypes.data, cnt.ctypes.data))
        return ids, dist, cnt

    def queryWithDistance(self, embedding: np.ndarray, numOfNeighbours: int, runtimeParams: Optional[AnnoyRuntimeParams] = None) -> List[Tuple[int, float]]:
        """RawAnnoyQueryIndex.scala:98-119: neighboursToRequest neighbours are asked of the library (its search_k is numOfTrees
        times that) and the first numOfNeighbours are kept.  Here the budget goes to the walk and k stays numOfNeighbours: the
        k best of a set are the first k of its best k'."""
        nte = None if runtimeParams is None else runtimeParams.nodesToExplore
        ids, dist, cnt = self.search(np.asarray(embedding, np.float32)[None, :], numOfNeighbours, nte)
        return [(int(ids[0, i]), float(dist[0, i])) for i in range(cnt[0])]

    def query(self, embedding: np.ndarray, numOfNeighbours: int, runtimeParams: Optional[AnnoyRuntimeParams] = None) -> List[int]:
        return [i for i, _ in self.queryWithDistance(embedding, numOfNeighbours, runtimeParams)]

    def forest(self) -> AnnoyForest:
        """The index's forest, borrowed: valid while the index is open."""
        lib = _lib()
        h = C.c_void_p()
        _check(lib, lib.annoy_index_forest(self._h, C.byref(h)))
        return AnnoyForest(h, owned=False, keeper=self)

    def rows(self, row0: int = 0, m: Optional[int] = None) -> np.ndarray:
        """The stored rows [row0, row0 + m): float16 [m, d]."""
        if m is None:
            m = self.n - row0
        out = np.empty((m, self.d), np.float16)
        lib = _lib()
        _check(lib, lib.annoy_index_get_rows(self._h, row0, m, out.ctypes.data))
        return out

    def last_candidates(self) -> Tuple[np.ndarray, np.ndarray]:
        """(positions int32 [nq, width], counts [nq]) of the last search: the distinct positions, ascending; -1 past the count."""
        nq, width = C.c_int32(), C.c_int32()
        lib = _lib()
        _check(lib, lib.annoy_last_candidates(self._h, C.byref(nq), C.byref(width), None, None))
        pos = np.full((nq.value, width.value), -1, np.int32)
        cnt = np.zeros(nq.value, np.int32)
        _check(lib, lib.annoy_last_candidates(self._h, None, None, pos.ctypes.data, cnt.ctypes.data))
        return pos, cnt

    def last_stats(self) -> dict:
        nq = C.c_int32()
        lib = _lib()
        _check(lib, lib.annoy_last_candidates(self._h, C.byref(nq), None, None, None))
        pops, coll = np.zeros(nq.value, np.int32), np.zeros(nq.value, np.int32)
        rerun, slices = C.c_int32(), C.c_int32()
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        _check(lib, lib.annoy_last_stats(self._h, pops.ctypes.data, coll.ctypes.data, C.byref(rerun), C.byref(slices), C.byref(a),
                                         C.byref(b), C.byref(c)))
        return {"pops": pops, "collected": coll, "rerun": rerun.value, "slices": slices.value, "walk_ms": a.value,
                "score_ms": b.value, "select_ms": c.value}

    def debug_set_limits(self, first_queue_capacity: int = 0, scratch_budget_bytes: int = 0) -> None:
        lib = _lib()
        _check(lib, lib.annoy_debug_set_limits(self._h, first_queue_capacity, scratch_budget_bytes))


class RawAnnoyIndexBuilder:
    """RawAnnoyIndexBuilder.scala: append(embedding) returns the counter 1, 2, ..., which is the item's id; toQueryable()
    builds the forest and ends the builder."""

    def __init__(self, dimension: int, numOfTrees: int, metric, *, leaf_size: int = 0, seed: int = 1, threads: int = 0, device: int = 0):
        self.metric = _metric(metric)
        if not 1 <= dimension <= MAX_D:
            raise ValueError(f"dimension must be in 1..{MAX_D}")
        if not 1 <= numOfTrees <= MAX_TREES:
            raise ValueError(f"numOfTrees must be in 1..{MAX_TREES}")
        self.dimension, self.numOfTrees = dimension, numOfTrees
        self._opts = dict(leaf_size=leaf_size, seed=seed, threads=threads, device=device)
        self._rows: Optional[List[np.ndarray]] = []

    def append(self, embedding) -> int:
        if self._rows is None:
            raise AnnoyError("the builder has ended: toQueryable() was called")
        v = np.asarray(embedding, np.float32)
        if v.shape != (self.dimension,):
            raise ValueError(f"expected an embedding of dimension {self.dimension}, got shape {v.shape}")
        self._rows.append(v)
        return len(self._rows)

    def _ids(self):
        return None

    def toQueryable(self) -> AnnoyQueryable:
        if self._rows is None:
            raise AnnoyError("the builder has ended: toQueryable() was called")
        if not self._rows:
            raise AnnoyError("no embedding was appended")
        rows, ids = np.stack(self._rows), self._ids()
        self._rows = None
        return AnnoyQueryable.build(self.metric, rows, self.numOfTrees, ids, **self._opts)


class _TypedAnnoyIndexBuilder(RawAnnoyIndexBuilder):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._caller_ids: List[int] = []

    def append(self, entity_id: int, embedding=None) -> int:  # EntityEmbedding(id, embedding)
        n = super().append(embedding)
        self._caller_ids.append(int(entity_id))
        return n

    def _ids(self):
        return np.asarray(self._caller_ids, np.int64)


class TypedAnnoyIndex:
    """TypedAnnoyIndex.scala: the raw index behind a map from the counter to the caller's ids (int64 here; the injection of
    the reference is the caller's)."""

    @staticmethod
    def indexBuilder(dimension: int, numOfTrees: int, metric, **kwargs) -> _TypedAnnoyIndexBuilder:
        return _TypedAnnoyIndexBuilder(dimension, numOfTrees, metric, **kwargs)
