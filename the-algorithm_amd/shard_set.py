"""ctypes binding of include/shard_set.h: several loaded Faiss-style indexes served as one, merged on the device.

Reference (paths relative to the reference's ann/src/main/scala/com/twitter/ann/):
  service/query_server/faiss/FaissQueryIndexServer.scala:102-112   --sharded
  faiss/HourlyShardedIndex.scala:66-93                             the newest hourly directories as one IndexShards
The members are FaissIvfFlat, FaissIvfPq and FaissOpqIvfPq objects (or their Polysemous twins) that the caller goes on
owning; faiss_files.HourlyShardedIndex is the holder the reference has.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple

import numpy as np

from . import binding as _binding
from .dense_ann import DistanceMetric
from .ivf_ann import KIND_IVF_FLAT, KIND_IVF_PQ, KIND_OPQ_IVF_PQ, FaissIvfFlat, IvfError, _rows  # noqa: F401
from .ivfpq_ann import FaissIvfPq  # noqa: F401
from .opq_ann import FaissOpqIvfPq  # noqa: F401
from .simclusters_ann import load_library

_P = C.POINTER
PROTOS = {
    "shardset_last_error": (C.c_char_p, []),
    "shardset_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P(C.c_void_p)]),
    "shardset_set_members": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "shardset_info": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), _P(C.c_int32), _P(C.c_int64)]),
    "shardset_search": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "shardset_last_stats": (C.c_int, [C.c_void_p, _P(C.c_int64), _P(C.c_int64), _P(C.c_int64), _P(C.c_float), _P(C.c_float)]),
    "shardset_compose": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "shardset_destroy": (C.c_int, [C.c_void_p]),
}



class ShardSetError(IvfError):
    """A status other than 0 from shard_set.h; `code` is the status (1 = IVF_EINVAL)."""

    def __init__(self, code: int, message: str):
        super().__init__(f"shard_set error {code}: {message}")
        self.code, self.message = code, message


_lib = _binding.binder(PROTOS, "shard_set", load_library)
_check = _binding.checker(ShardSetError, "shard_set", "shardset_last_error", with_code=True)
_ptr = _binding.ptr


def kind_of(index) -> int:
    """The FAISS_KIND_* of an index object of the three families."""
    kind = getattr(index, "FAISS_KIND", None)
    if kind not in (KIND_IVF_FLAT, KIND_IVF_PQ, KIND_OPQ_IVF_PQ):
        raise TypeError(f"{type(index).__name__} is not one of FaissIvfFlat, FaissIvfPq, FaissOpqIvfPq")
    return kind


class ShardSet(_binding.Handle):
    """shard_set.h: create(), set_members() with loaded indexes (newest first), search().  The set keeps a reference to
    every member object, so a member is not collected while it serves; closing a member is the caller's, after it has
    left the set."""

    _destroy, _lib = "shardset_destroy", staticmethod(_lib)

    def __init__(self, handle, metric: DistanceMetric, dimension: int, device: int):
        self._h, self.metric, self.dimension, self.device = handle, DistanceMetric(metric), int(dimension), device
        self._members: List[object] = []

    @classmethod
    def create(cls, metric: DistanceMetric, dimension: int, *, device: int = 0):
        lib = _lib()
        h = C.c_void_p()
        _check(lib, lib.shardset_create(device, int(dimension), int(metric), C.byref(h)))
        return cls(h, metric, dimension, device)

    @property
    def members(self) -> List[object]:
        return list(self._members)

    def set_members(self, indexes: Sequence[object]) -> None:
        """Replaces the whole membership (shardset_set_members).  A refusal leaves the membership as it was."""
        lib = _lib()
        indexes = list(indexes)
        n = len(indexes)
        kinds = (C.c_int32 * max(n, 1))(*[kind_of(ix) for ix in indexes])
        handles = (C.c_void_p * max(n, 1))(*[ix._h.value if isinstance(ix._h, C.c_void_p) else ix._h for ix in indexes])
        _check(lib, lib.shardset_set_members(self._h, n, C.cast(kinds, C.c_void_p), C.cast(handles, C.c_void_p)))
        self._members = indexes

    def info(self) -> dict:
        lib = _lib()
        n, d, m, rows = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        _check(lib, lib.shardset_info(self._h, C.byref(n), C.byref(d), C.byref(m), C.byref(rows)))
        return {"members": n.value, "dimension": d.value, "metric": DistanceMetric(m.value), "rows": rows.value}

    def search(self, queries: np.ndarray, k: int, nprobe: int, ht: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(ids [nq, k], distances [nq, k], counts [nq]): for each query the best k of all members' answers by (distance,
        id) -- the bytes of dense_ann.compose over the members' own searches."""
        lib = _lib()
        q = _rows(queries, self.dimension)
        nq = q.shape[0]
        ids, dist, cnt = _binding.result_triple(nq, k, clamp=True)
        _check(lib, lib.shardset_search(self._h, nq, _ptr(q), k, nprobe, int(ht), _ptr(dist), _ptr(ids), _ptr(cnt)))
        return ids, dist, cnt

    def last_stats(self) -> dict:
        lib = _lib()
        h2d, d2h, res = C.c_int64(), C.c_int64(), C.c_int64()
        ts, tf = C.c_float(), C.c_float()
        _check(lib, lib.shardset_last_stats(self._h, C.byref(h2d), C.byref(d2h), C.byref(res), C.byref(ts), C.byref(tf)))
        return {"h2d_bytes": h2d.value, "d2h_bytes": d2h.value, "d2h_result_bytes": res.value, "search_ms": ts.value,
                "fold_ms": tf.value}

    @staticmethod
    def compose(shard_results: Sequence[Tuple[np.ndarray, np.ndarray, np.ndarray]], k: int, *, device: int = 0):
        """dense_ann.compose through the fold kernel (shardset_compose): every shard's (ids, distances, counts), each
        [nq, k_in] / [nq] with one k_in, ordered by (distance, id), the best k kept."""
        lib = _lib()
        s_ids = np.ascontiguousarray(np.stack([np.asarray(r[0], np.int64) for r in shard_results]))
        s_dist = np.ascontiguousarray(np.stack([np.asarray(r[1], np.float32) for r in shard_results]))
        s_cnt = np.ascontiguousarray(np.stack([np.asarray(r[2], np.int32) for r in shard_results]))
        n_shards, nq, k_in = s_ids.shape
        ids, dist, cnt = _binding.result_triple(nq, k, clamp=True)
        _check(lib, lib.shardset_compose(device, n_shards, nq, k_in, _ptr(s_ids), _ptr(s_dist), _ptr(s_cnt), k, _ptr(ids), _ptr(dist),
                                         _ptr(cnt)))
        return ids, dist, cnt

    def _closed(self) -> None:
        self._members = []
