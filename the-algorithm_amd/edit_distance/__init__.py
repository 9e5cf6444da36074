"""ctypes binding of include/edit_ann.h: the EditDistance metric of the reference's ann/ and the exhaustive index under it.

Reference (paths relative to the reference's ann/src/main/):
  scala/com/twitter/ann/common/Metric.scala:187-261                Metric.Edit: Levenshtein distance over Seq[Float]
  scala/com/twitter/ann/common/EmbeddingType.scala                  EditDistance(distance: Int), the distance value type
  thrift/com/twitter/ann/common/ann_common.thrift:16-19, 107-121   DistanceMetric.EditDistance = 7; Distance arm 4, an i32
  scala/com/twitter/ann/brute_force/BruteForceIndex.scala:40-91    append, query, queryWithDistance
An embedding is a variable-length sequence of floats, one per character (encode_strings makes them from Python strings, one
float per code point).  Batches of strings travel as CSR: (offsets int64 [n + 1], chars fp32).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .. import binding as _binding
from ..simclusters_ann import load_library

_P = C.POINTER
_CSR = [C.c_void_p, C.c_void_p, C.c_int64]  # offsets, chars, n_chars
PROTOS = {
    "edit_last_error": (C.c_char_p, []),
    "edit_index_build": (C.c_int, [C.c_int32, C.c_int64] + _CSR + [C.c_void_p, _P(C.c_void_p)]),
    "edit_index_append": (C.c_int, [C.c_void_p, C.c_int64] + _CSR + [C.c_void_p]),
    "edit_index_reserve": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64]),
    "edit_index_info": (C.c_int, [C.c_void_p, _P(C.c_int64), _P(C.c_int64), _P(C.c_int32)]),
    "edit_index_get_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, _P(C.c_int64), C.c_void_p]),
    "edit_index_destroy": (None, [C.c_void_p]),
    "edit_search": (C.c_int, [C.c_void_p, C.c_int64] + _CSR + [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "edit_pair_distances": (C.c_int, [C.c_int32, C.c_int64] + _CSR + _CSR + [C.c_void_p]),
    "edit_pair_distances_host": (C.c_int, [C.c_int64] + _CSR + _CSR + [C.c_void_p]),
    "edit_index_set_query_slice": (C.c_int, [C.c_void_p, C.c_int32]),
    "edit_last_timing": (C.c_int, [C.c_void_p, _P(C.c_float), _P(C.c_float)]),
    "edit_last_stats": (C.c_int, [C.c_void_p, _P(C.c_int64), _P(C.c_int64)]),
    "edit_wire_encode_neighbor_result": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, _P(C.c_int64)]),
    "edit_wire_decode_neighbor_result": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, _P(C.c_int32),
                                                   _P(C.c_int64)]),
}

EDIT_OK, EDIT_EINVAL, EDIT_EDEVICE, EDIT_ELIMIT, EDIT_ENOMEM, EDIT_EINTERNAL, EDIT_ESPACE, EDIT_EFORMAT = range(8)
DISTANCE_METRIC_EDIT = 7  # DistanceMetric.EditDistance
MAX_LENGTH = 256
MAX_K = 1024


class EditError(RuntimeError):
    """A refusal of the library: `code` is the EDIT_* status."""

    def __init__(self, code: int, message: str):
        super().__init__(f"edit_ann error {code}: {message}")
        self.code = code


_lib = _binding.binder(PROTOS, "edit", load_library)
_check = _binding.checker(EditError, "edit_ann", "edit_last_error", with_code=True)


class EditDistance(int):
    """The distance value type (the reference's EditDistance(distance: Int)): an int that orders and compares as one."""

    @property
    def distance(self) -> int:
        return int(self)

    def __repr__(self) -> str:
        return f"EditDistance({int(self)})"


def encode_strings(strings: Sequence[str]) -> List[np.ndarray]:
    """One fp32 array per string, one float per code point (every code point is exact in fp32: they end at 0x10FFFF)."""
    return [np.array([ord(c) for c in s], np.float32) for s in strings]


def _embedding(e) -> np.ndarray:
    if isinstance(e, str):
        return encode_strings([e])[0]
    return np.ascontiguousarray(e, np.float32).reshape(-1)


def to_csr(rows) -> Tuple[np.ndarray, np.ndarray]:
    """(offsets int64 [n + 1], chars fp32) of a sequence of embeddings (float arrays or strings); an (offsets, chars) pair of
    arrays with int64 offsets passes through."""
    if isinstance(rows, tuple) and len(rows) == 2 and isinstance(rows[0], np.ndarray) and rows[0].dtype == np.int64:
        return np.ascontiguousarray(rows[0], np.int64), np.ascontiguousarray(rows[1], np.float32).reshape(-1)
    arrays = [_embedding(r) for r in rows]
    offsets = np.zeros(len(arrays) + 1, np.int64)
    if arrays:
        np.cumsum([a.size for a in arrays], out=offsets[1:])
    return offsets, (np.concatenate(arrays) if arrays else np.zeros(0, np.float32))


def from_csr(offsets: np.ndarray, chars: np.ndarray) -> List[np.ndarray]:
    return [chars[offsets[i]:offsets[i + 1]].copy() for i in range(len(offsets) - 1)]


def _csr_args(offsets: np.ndarray, chars: np.ndarray):
    return offsets.ctypes.data, (chars.ctypes.data if chars.size else None), chars.size


class Edit:
    """The metric (Metric.Edit).  distance: one pair, on the host; distances: a batch of pairs, on the host (device=None) or
    on a device, through the distance function of the search."""

    @staticmethod
    def distance(a, b) -> EditDistance:
        return EditDistance(Edit.distances([(a, b)])[0])

    @staticmethod
    def distances(pairs, device: Optional[int] = None) -> np.ndarray:
        pairs = list(pairs)
        ao, ac = to_csr([a for a, _ in pairs])
        bo, bc = to_csr([b for _, b in pairs])
        return pair_distances(ao, ac, bo, bc, device)

    @staticmethod
    def from_absolute_distance(distance: float) -> EditDistance:
        return EditDistance(int(distance))


def pair_distances(a_offsets, a_chars, b_offsets, b_chars, device: Optional[int] = None) -> np.ndarray:
    """int32 [n]: the distance of a[i] to b[i] for two CSR batches of one length."""
    lib = _lib()
    ao, ac = to_csr((np.ascontiguousarray(a_offsets, np.int64), a_chars))
    bo, bc = to_csr((np.ascontiguousarray(b_offsets, np.int64), b_chars))
    if ao.shape != bo.shape or ao.ndim != 1 or ao.size < 1:
        raise ValueError("a and b hold one string per pair")
    n = ao.size - 1
    out = np.zeros(n, np.int32)
    if device is None:
        _check(lib, lib.edit_pair_distances_host(n, *_csr_args(ao, ac), *_csr_args(bo, bc), out.ctypes.data))
    else:
        _check(lib, lib.edit_pair_distances(int(device), n, *_csr_args(ao, ac), *_csr_args(bo, bc), out.ctypes.data))
    return out


_NO_IDS = np.zeros(1, np.int64)  # a non-NULL address for an empty id array


def _ids_arg(ids, n: int):
    idp = _binding.ids_or_none(ids, n, "row")
    return idp, (None if idp is None else idp.ctypes.data if n else _NO_IDS.ctypes.data)


class EditBruteForceIndex(_binding.Handle):
    """BruteForceIndex under Metric.Edit on the device.  rows: a sequence of embeddings (float arrays, or strings), or a CSR
    pair.  ids None: the ids are positions, and append takes none either."""

    _destroy = "edit_index_destroy"
    _lib = staticmethod(_lib)

    def __init__(self, rows=(), ids=None, device: int = 0):
        lib = _lib()
        off, ch = to_csr(rows)
        idp, ida = _ids_arg(ids, off.size - 1)
        h = C.c_void_p()
        _check(lib, lib.edit_index_build(int(device), off.size - 1, *_csr_args(off, ch), ida, C.byref(h)))
        self._h = h
        self.device = int(device)

    def append(self, rows, ids=None) -> None:
        lib = _lib()
        off, ch = to_csr(rows)
        idp, ida = _ids_arg(ids, off.size - 1)
        _check(lib, lib.edit_index_append(self._h, off.size - 1, *_csr_args(off, ch), ida))

    def reserve(self, rows: int, total_chars: int) -> None:
        lib = _lib()
        _check(lib, lib.edit_index_reserve(self._h, int(rows), int(total_chars)))

    def info(self) -> dict:
        lib = _lib()
        n, c, m = C.c_int64(), C.c_int64(), C.c_int32()
        _check(lib, lib.edit_index_info(self._h, C.byref(n), C.byref(c), C.byref(m)))
        return {"n": n.value, "total_chars": c.value, "max_len": m.value}

    def __len__(self) -> int:
        return self.info()["n"]

    def rows(self, i0: int = 0, n: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Audit: (offsets, chars, ids) of rows i0 .. i0 + n in arrival order, the stored bits."""
        lib = _lib()
        n = len(self) - i0 if n is None else n
        need = C.c_int64()
        off, ids = np.zeros(max(n, 0) + 1, np.int64), np.zeros(max(n, 0), np.int64)
        _check(lib, lib.edit_index_get_rows(self._h, i0, n, off.ctypes.data, None, 0, C.byref(need), ids.ctypes.data))
        chars = np.zeros(need.value, np.float32)
        _check(lib, lib.edit_index_get_rows(self._h, i0, n, off.ctypes.data, chars.ctypes.data, chars.size, C.byref(need), ids.ctypes.data))
        return off, chars, ids

    def search(self, queries, k: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(dist int32 [nq, k], ids int64 [nq, k], counts int32 [nq]); entries past a count hold -1."""
        lib = _lib()
        off, ch = to_csr(queries)
        nq, width = off.size - 1, max(int(k), 0)
        dist, ids, counts = np.zeros((nq, width), np.int32), np.zeros((nq, width), np.int64), np.zeros(nq, np.int32)
        _check(lib, lib.edit_search(self._h, nq, *_csr_args(off, ch), int(k), dist.ctypes.data, ids.ctypes.data, counts.ctypes.data))
        return dist, ids, counts

    def query_with_distance(self, embedding, k: int) -> List[Tuple[int, EditDistance]]:
        """Queryable.queryWithDistance: [(id, EditDistance)], nearest first."""
        dist, ids, counts = self.search([_embedding(embedding)], k)
        return [(int(ids[0, i]), EditDistance(dist[0, i])) for i in range(counts[0])]

    def query(self, embedding, k: int) -> List[int]:
        """Queryable.query: the ids, nearest first."""
        return [i for i, _ in self.query_with_distance(embedding, k)]

    def set_query_slice(self, max_queries_per_pass: int) -> None:
        lib = _lib()
        _check(lib, lib.edit_index_set_query_slice(self._h, int(max_queries_per_pass)))

    def last_timing(self) -> dict:
        lib = _lib()
        a, b = C.c_float(), C.c_float()
        _check(lib, lib.edit_last_timing(self._h, C.byref(a), C.byref(b)))
        return {"distance_ms": a.value, "select_ms": b.value}

    def last_stats(self) -> dict:
        lib = _lib()
        a, b = C.c_int64(), C.c_int64()
        _check(lib, lib.edit_last_stats(self._h, C.byref(a), C.byref(b)))
        return {"pairs": a.value, "cell_updates": b.value}


def encode_neighbor_result(ids, distances=None) -> bytes:
    """NearestNeighborResult in TBinaryProtocol with the editDistance arm (distances None: ids only)."""
    lib = _lib()
    idp = np.ascontiguousarray(ids, np.int64).reshape(-1)
    dp = None if distances is None else np.ascontiguousarray(distances, np.int32).reshape(-1)
    if dp is not None and dp.shape != idp.shape:
        raise ValueError("one distance per id")
    n = C.c_int64()
    rc = lib.edit_wire_encode_neighbor_result(idp.size, idp.ctypes.data, _binding.ptr(dp), None, 0, C.byref(n))  # the size
    if rc != EDIT_ESPACE:
        _check(lib, rc)
    buf = np.zeros(n.value, np.uint8)
    _check(lib, lib.edit_wire_encode_neighbor_result(idp.size, idp.ctypes.data, _binding.ptr(dp), buf.ctypes.data, buf.size, C.byref(n)))
    return buf.tobytes()


def decode_neighbor_result(data: bytes) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(ids int64, distances int32, arms int32) -- arm 4 where the neighbour carried an editDistance, else 0."""
    lib = _lib()
    buf = np.frombuffer(bytes(data) + b"\0", np.uint8)  # (a non-NULL address for an empty message)
    count, used = C.c_int32(), C.c_int64()
    _check(lib, lib.edit_wire_decode_neighbor_result(buf.ctypes.data, len(data), 0, None, None, None, C.byref(count), C.byref(used)))
    ids, dist, arms = np.zeros(count.value, np.int64), np.zeros(count.value, np.int32), np.zeros(count.value, np.int32)
    _check(lib, lib.edit_wire_decode_neighbor_result(buf.ctypes.data, len(data), count.value, ids.ctypes.data, dist.ctypes.data, arms.ctypes.data,
                                                     C.byref(count), C.byref(used)))
    return ids, dist, arms
