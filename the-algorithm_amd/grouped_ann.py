"""ctypes binding of include/grouped_ann.h and a host-side mirror of the reference's grouped query path.

Reference (paths relative to the reference's ann/src/main/):
  scala/com/twitter/ann/dataflow/offline/ANNIndexBuilderBeamJob.scala:192-216,247-268   transformTableRowToKeyVal, groupBy(_.getKey)
  scala/com/twitter/ann/common/Api.scala:54-88                                          QueryableGrouped
  scala/com/twitter/ann/service/query_server/common/RefreshableQueryable.scala:47-55,131-177
                                                                                        Map[Option[String], Queryable]
  scala/com/twitter/ann/service/query_server/common/QueryIndexThriftController.scala:42-57   query.key
The device knows group numbers only; the key <-> group-number table lives here, in first-appearance order.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import binding as _binding
from .dense_ann import DistanceMetric
from .simclusters_ann import load_library

_P = C.POINTER
PROTOS = {
    "gann_last_error": (C.c_char_p, []),
    "gann_index_build": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                   _P(C.c_void_p)]),
    "gann_search": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gann_index_info": (C.c_int, [C.c_void_p, _P(C.c_int64), _P(C.c_int32), _P(C.c_int32), _P(C.c_int32)]),
    "gann_index_group_sizes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gann_last_stats": (C.c_int, [C.c_void_p, _P(C.c_int64), _P(C.c_int64), _P(C.c_int32), _P(C.c_int64), _P(C.c_int32),
                                  _P(C.c_float), _P(C.c_float), _P(C.c_float)]),
    "gann_index_destroy": (C.c_int, [C.c_void_p]),
}

FLAT_KEY = ""  # the key of data without groups (ANNIndexBuilderBeamJob.scala:255-259)


class GroupedError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"grouped_ann error {code}: {message}")
        self.code = code


_lib = _binding.binder(PROTOS, "gann", load_library)
_check = _binding.checker(GroupedError, "grouped_ann", "gann_last_error", with_code=True)
_rows = _binding.rows


def key_table(keys: Sequence[str]) -> Tuple[List[str], np.ndarray]:
    """Keys of the rows -> (the distinct keys in first-appearance order, the group number of every row: int32)."""
    table: Dict[str, int] = {}
    groups = np.empty(len(keys), np.int32)
    for i, key in enumerate(keys):
        groups[i] = table.setdefault(key, len(table))
    return list(table), groups


def group_rows(entity_ids: Sequence[Optional[int]], embeddings: Sequence[Sequence[float]],
               group_ids: Optional[Sequence[str]] = None) -> Dict[str, List[Tuple[int, np.ndarray]]]:
    """transformTableRowToKeyVal + groupBy(_.getKey) (ANNIndexBuilderBeamJob.scala:211-216,247-268): a row without an
    entity id is dropped; the key is the row's group id, or "" for data without groups; the embedding becomes fp32.  The
    keys are in first-appearance order, and so are the rows of a key."""
    if len(entity_ids) != len(embeddings) or (group_ids is not None and len(group_ids) != len(entity_ids)):
        raise ValueError("one embedding (and one group id) per entity id")
    out: Dict[str, List[Tuple[int, np.ndarray]]] = {}
    for i, eid in enumerate(entity_ids):
        if eid is None:
            continue
        key = FLAT_KEY if group_ids is None else group_ids[i]
        if key is None:
            raise ValueError(f"row {i}: grouped data without a group id")
        out.setdefault(key, []).append((int(eid), np.asarray(embeddings[i], np.float32)))
    return out


class GroupedIndex(_binding.Handle):
    """All groups in one index resident in HBM; search() answers every query from the rows of its own key."""

    _destroy, _lib = "gann_index_destroy", staticmethod(_lib)

    def __init__(self, handle, metric: DistanceMetric, d: int, keys: List[str]):
        self._h, self.metric, self.d = handle, DistanceMetric(metric), d
        self.keys = list(keys)
        self._number = {key: g for g, key in enumerate(self.keys)}

    @classmethod
    def build_numbered(cls, vectors: np.ndarray, ids: Optional[Sequence[int]], groups: Sequence[int], keys: Sequence[str],
                       metric: DistanceMetric, device: int = 0):
        """groups: the group number of every row, in [0, len(keys)); keys: the key of every group number (a group may be
        empty).  ids: one int64 per row, or None (ids = positions)."""
        lib = _lib()
        v = _rows(vectors)
        g = np.ascontiguousarray(groups, np.int32)
        if g.shape != (v.shape[0],):
            raise ValueError("one group per vector")
        idp = _binding.ids_or_none(ids, v.shape[0])
        h = C.c_void_p()
        _check(lib, lib.gann_index_build(device, int(metric), v.shape[1], len(keys), v.shape[0], v.ctypes.data,
                                         _binding.ptr(idp), g.ctypes.data, C.byref(h)))
        return cls(h, metric, v.shape[1], list(keys))

    @classmethod
    def build(cls, vectors: np.ndarray, ids: Optional[Sequence[int]], keys: Sequence[str], metric: DistanceMetric, device: int = 0):
        """keys: one string per row; the group numbers are the keys' ranks in first-appearance order.  ids: one int64 per
        row, or None (ids = positions)."""
        if len(keys) != len(vectors):
            raise ValueError("one key per vector")
        table, groups = key_table(keys)
        return cls.build_numbered(vectors, ids, groups, table, metric, device)

    def group_numbers(self, keys: Sequence[Optional[str]]) -> np.ndarray:
        """The group number of every key: -1 for None and for a key that is not in the index."""
        return np.array([-1 if key is None else self._number.get(key, -1) for key in keys], np.int32)

    def search_groups(self, queries: np.ndarray, groups: Sequence[int], k: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """search() with group numbers in place of keys."""
        lib = _lib()
        q = _rows(queries, self.d)
        nq = q.shape[0]
        g = np.ascontiguousarray(groups, np.int32)
        if g.shape != (nq,):
            raise ValueError("one group per query")
        ids, dist, cnt = _binding.result_triple(nq, k)
        _check(lib, lib.gann_search(self._h, nq, q.ctypes.data, g.ctypes.data, k, dist.ctypes.data, ids.ctypes.data, cnt.ctypes.data))
        return ids, dist, cnt

    def search(self, queries: np.ndarray, keys: Sequence[Optional[str]], k: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(ids [nq, k], distances [nq, k], counts [nq]): the exact k nearest rows of each query's key, ascending by
        (distance, id); counts = min(k, rows of the key), 0 for None and for a key that is not in the index."""
        return self.search_groups(queries, self.group_numbers(keys), k)

    def info(self) -> dict:
        n, d, m, g = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
        lib = _lib()
        _check(lib, lib.gann_index_info(self._h, C.byref(n), C.byref(d), C.byref(m), C.byref(g)))
        return {"n": n.value, "d": d.value, "metric": m.value, "n_groups": g.value}

    def group_sizes(self) -> np.ndarray:
        out = np.empty(len(self.keys), np.int64)
        lib = _lib()
        _check(lib, lib.gann_index_group_sizes(self._h, out.ctypes.data))
        return out

    def last_stats(self) -> dict:
        tiles, work, rows = C.c_int64(), C.c_int64(), C.c_int64()
        rounds, seg = C.c_int32(), C.c_int32()
        a, b, s = C.c_float(), C.c_float(), C.c_float()
        lib = _lib()
        _check(lib, lib.gann_last_stats(self._h, C.byref(tiles), C.byref(work), C.byref(rounds), C.byref(rows), C.byref(seg),
                                        C.byref(a), C.byref(b), C.byref(s)))
        return {"tiles": tiles.value, "work_items": work.value, "rounds": rounds.value, "rows_scanned": rows.value,
                "segment_rows": seg.value, "worklist_ms": a.value, "scan_ms": b.value, "select_ms": s.value}


class GroupedQueryable:
    """QueryableGrouped (Api.scala:54-85) as RefreshableQueryable serves it (:131-167) on top of GroupedIndex.search.

    `runtime_params` is accepted and ignored: the search is exact within the group, which is the upper bound of what the
    reference's per-group HNSW or Faiss index would find under any of its runtime parameters.  A key that is not in the
    index answers [], and so does a key of None: a grouped mapping has no None entry (RefreshableQueryable.scala:48-51,139)."""

    def __init__(self, index: GroupedIndex):
        self.index = index

    def batch_query_with_distance(self, embeddings: np.ndarray, num_neighbors: int, runtime_params=None,
                                  keys: Optional[Sequence[Optional[str]]] = None) -> List[List[Tuple[int, float]]]:
        q = _rows(embeddings, self.index.d)
        if keys is None:
            keys = [None] * q.shape[0]
        ids, dist, cnt = self.index.search(q, keys, num_neighbors)
        return [list(zip(ids[i, :cnt[i]].tolist(), dist[i, :cnt[i]].tolist())) for i in range(q.shape[0])]

    def batch_query(self, embeddings: np.ndarray, num_neighbors: int, runtime_params=None,
                    keys: Optional[Sequence[Optional[str]]] = None) -> List[List[int]]:
        return [[i for i, _ in row] for row in self.batch_query_with_distance(embeddings, num_neighbors, runtime_params, keys)]

    def query_with_distance(self, embedding: np.ndarray, num_neighbors: int, runtime_params=None,
                            key: Optional[str] = None) -> List[Tuple[int, float]]:
        return self.batch_query_with_distance(np.asarray(embedding, np.float32)[None, :], num_neighbors, runtime_params, [key])[0]

    def query(self, embedding: np.ndarray, num_neighbors: int, runtime_params=None, key: Optional[str] = None) -> List[int]:
        return [i for i, _ in self.query_with_distance(embedding, num_neighbors, runtime_params, key)]
