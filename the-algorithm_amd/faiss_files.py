"""ctypes binding of include/faiss_files.h and a host-side mirror of how the reference writes, reads and serves its Faiss
indexes.

Reference (paths relative to the reference's ann/src/main/scala/com/twitter/ann/faiss/):
  FaissIndexer.scala:68-110                          buildAndWriteFaissIndex: build, write faiss.index, then _SUCCESS
  FaissIndex.scala:28-, QueryableIndexAdapter.scala:19-31   loadIndex(dimension, metric, directory)
  FaissCommon.scala:39-43                            isValidFaissIndex
  HourlyDirectoryWithSuccessFileListing.scala:16-63  the newest hourly directories that carry a success file
  HourlyShardedIndex.scala:59-93                     reloadShards: the fresh set of directories as one IndexShards
The file is the project's own container (faiss_files.h says why); native Faiss files are not read.
"""
from __future__ import annotations

import ctypes as C
import datetime as _dt
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import binding as _binding
from . import dense_ann, opq_ann, polysemous_ann
from .dense_ann import DistanceMetric
from .ivf_ann import KIND_IVF_FLAT, KIND_IVF_PQ, KIND_OPQ_IVF_PQ, FaissIvfFlat, FaissQueryable, IvfError, _rows  # noqa: F401
from .ivfpq_ann import KSUB, FaissIvfPq
from .opq_ann import FaissOpqIvfPq
from .shard_set import ShardSet
from .simclusters_ann import load_library

_P = C.POINTER
PROTOS = {
    "faiss_last_error": (C.c_char_p, []),
    "faiss_file_write": (C.c_int, [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "faiss_file_open": (C.c_int, [C.c_char_p, _P(C.c_void_p)]),
    "faiss_file_info": (C.c_int, [C.c_void_p, _P(C.c_int32), _P(C.c_int32), _P(C.c_int32), _P(C.c_int32), _P(C.c_int32),
                                  _P(C.c_int32), _P(C.c_int32), _P(C.c_int64)]),
    "faiss_file_read_centroids": (C.c_int, [C.c_void_p, C.c_void_p]),
    "faiss_file_read_codebooks": (C.c_int, [C.c_void_p, C.c_void_p]),
    "faiss_file_read_matrix": (C.c_int, [C.c_void_p, C.c_void_p]),
    "faiss_file_read_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "faiss_file_close": (C.c_int, [C.c_void_p]),
    "faiss_directory_is_valid": (C.c_int, [C.c_char_p]),
    "faiss_ivf_index_save_directory": (C.c_int, [C.c_void_p, C.c_char_p]),
    "faiss_ivfpq_index_save_directory": (C.c_int, [C.c_void_p, C.c_char_p]),
    "faiss_opq_index_save_directory": (C.c_int, [C.c_void_p, C.c_char_p]),
    "faiss_index_load_directory": (C.c_int, [C.c_int32, C.c_char_p, C.c_int32, C.c_int32, _P(C.c_int32), _P(C.c_void_p)]),
    "faiss_ivf_index_get_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "faiss_index_ids_mode": (C.c_int, [C.c_int32, C.c_void_p, _P(C.c_int32)]),
}

IDS_POSITIONS, IDS_GIVEN, IDS_NONE = 0, 1, 2
INDEX_FILE_NAME = "faiss.index"
SUCCESS_FILE_NAME = "_SUCCESS"


class FaissFileError(IvfError):
    """A status other than 0 from faiss_files.h; `code` is the status (1 = IVF_EINVAL)."""

    def __init__(self, code: int, message: str):
        super().__init__(f"faiss_files error {code}: {message}")
        self.code, self.message = code, message


_lib = _binding.binder(PROTOS, "faiss_files", load_library)
_check = _binding.checker(FaissFileError, "faiss_files", "faiss_last_error", with_code=True)
_FAMILY = {cls.FAISS_KIND: cls for cls in (FaissIvfFlat, FaissIvfPq, FaissOpqIvfPq)}


def _path(p) -> bytes:
    return os.fsencode(os.fspath(p))


def _ptr(a: Optional[np.ndarray]):
    return _binding.ptr(None if a is None or a.size == 0 else a)


# ---- the file, host only ------------------------------------------------------------------------------------------------
def write_file(path, kind: int, metric: DistanceMetric, *, centroids: np.ndarray, ids_mode: int, ids: np.ndarray, cells: np.ndarray,
               payload: np.ndarray, codebooks: Optional[np.ndarray] = None, matrix: Optional[np.ndarray] = None) -> None:
    """A whole index file from host arrays (faiss_file_write): centroids [nlist, d]; codebooks [M, 256, d / M]; matrix
    [d, d_in]; ids int64 [n]; cells int32 [n]; payload float16 [n, d] (IVF-Flat) or uint8 [n, M].  The values are written as
    given."""
    lib = _lib()
    c = np.ascontiguousarray(centroids, np.float32)
    nlist, d = c.shape
    cb = None if codebooks is None else np.ascontiguousarray(codebooks, np.float32)
    a = None if matrix is None else np.ascontiguousarray(matrix, np.float32)
    i64 = np.ascontiguousarray(ids, np.int64).reshape(-1)
    c32 = np.ascontiguousarray(cells, np.int32).reshape(-1)
    n = i64.shape[0]
    if kind == KIND_IVF_FLAT:
        pl = np.ascontiguousarray(payload, np.float16).reshape(n, d)
        M = 0
    else:
        M = cb.shape[0]
        pl = np.ascontiguousarray(payload, np.uint8).reshape(n, M)
        if cb.shape != (M, KSUB, d // M):
            raise ValueError(f"expected codebooks of shape [M, {KSUB}, d / M], got {cb.shape}")
    if c32.shape[0] != n:
        raise ValueError("one cell per id")
    d_in = d
    if kind == KIND_OPQ_IVF_PQ:
        if a is None or a.ndim != 2 or a.shape[0] != d:
            raise ValueError("an OPQ file needs its matrix [d, d_in]")
        d_in = a.shape[1]
    _check(lib, lib.faiss_file_write(_path(path), kind, int(metric), d_in, d, nlist, M, ids_mode, n, _ptr(c), _ptr(cb), _ptr(a),
                                     _ptr(i64), _ptr(c32), _ptr(pl)))


def read_file(path, *, slab: int = 1 << 16) -> dict:
    """Opens, checks and reads a whole index file into host arrays (rows `slab` at a time): the keys of write_file's
    arguments, with kind, metric, d_in, d, nlist, M and n."""
    lib = _lib()
    h = C.c_void_p()
    _check(lib, lib.faiss_file_open(_path(path), C.byref(h)))
    try:
        v = [C.c_int32() for _ in range(7)]
        n = C.c_int64()
        _check(lib, lib.faiss_file_info(h, *[C.byref(x) for x in v], C.byref(n)))
        kind, metric, d_in, d, nlist, M, ids_mode = [x.value for x in v]
        n = n.value
        out = dict(kind=kind, metric=DistanceMetric(metric), d_in=d_in, d=d, nlist=nlist, M=M, ids_mode=ids_mode, n=n)
        out["centroids"] = np.empty((nlist, d), np.float32)
        _check(lib, lib.faiss_file_read_centroids(h, out["centroids"].ctypes.data))
        if kind != KIND_IVF_FLAT:
            out["codebooks"] = np.empty((M, KSUB, d // M), np.float32)
            _check(lib, lib.faiss_file_read_codebooks(h, out["codebooks"].ctypes.data))
        if kind == KIND_OPQ_IVF_PQ:
            out["matrix"] = np.empty((d, d_in), np.float32)
            _check(lib, lib.faiss_file_read_matrix(h, out["matrix"].ctypes.data))
        out["ids"] = np.empty(n, np.int64)
        out["cells"] = np.empty(n, np.int32)
        out["payload"] = np.empty((n, d), np.float16) if kind == KIND_IVF_FLAT else np.empty((n, M), np.uint8)
        for r0 in range(0, n, slab):
            m = min(slab, n - r0)
            _check(lib, lib.faiss_file_read_rows(h, r0, m, out["ids"][r0:].ctypes.data, out["cells"][r0:].ctypes.data,
                                                 out["payload"][r0:].ctypes.data))
        return out
    finally:
        lib.faiss_file_close(h)


# ---- directories --------------------------------------------------------------------------------------------------------
def is_valid_faiss_index(directory) -> bool:
    """FaissCommon.isValidFaissIndex (:39-43): a directory with a success file and a faiss.index."""
    return bool(_lib().faiss_directory_is_valid(_path(directory)))


def write_index(index, directory) -> None:
    """swigfaiss.write_index + copyToOutputAndCreateSuccess (FaissIndexer.scala:95-110): the index file under a temporary
    name, renamed to faiss.index, then the empty _SUCCESS.  A directory that holds a faiss.index is refused."""
    lib = _lib()
    if getattr(index, "FAISS_KIND", None) not in _FAMILY:
        raise TypeError(f"write_index: {type(index).__name__} is not one of FaissIvfFlat, FaissIvfPq, FaissOpqIvfPq")
    _check(lib, getattr(lib, f"faiss_{index._prefix}_index_save_directory")(index._h, _path(directory)))


def build_and_write_faiss_index(vectors: np.ndarray, ids: Sequence[int], sample_rate: float, factory_string: Optional[str],
                                metric: DistanceMetric, output_directory, *, niter: int = 0, niter_opq: int = 0, seed: int = 1,
                                device: int = 0) -> None:
    """FaissIndexer.buildAndWriteFaissIndex (:68-100) in full: index_factory, train on the first trainingSetSize rows,
    add_with_ids all rows, write the index and the success file to output_directory.  The index does not outlive the call."""
    index = opq_ann.build_faiss_index(vectors, ids, sample_rate, factory_string, metric, niter=niter, niter_opq=niter_opq, seed=seed,
                                      device=device)
    try:
        write_index(index, output_directory)
    finally:
        index.close()


def _kind_of(index) -> int:
    return getattr(index, "FAISS_KIND", KIND_IVF_FLAT)


def ids_mode(index) -> int:
    """IDS_POSITIONS, IDS_GIVEN or IDS_NONE (no row added yet) of an index of the three types."""
    lib = _lib()
    out = C.c_int32()
    _check(lib, lib.faiss_index_ids_mode(_kind_of(index), index._h, C.byref(out)))
    return out.value


def stored_rows(index: FaissIvfFlat) -> np.ndarray:
    """The rows an IVF-Flat index stores, in the order added: float16 [n, d], the bits as stored."""
    lib = _lib()
    n = index.n
    out = np.empty((n, index.d), np.float16)
    if n:
        _check(lib, lib.faiss_ivf_index_get_rows(index._h, 0, n, out.ctypes.data))
    return out


def load_native_index(dimension: int, metric: DistanceMetric, directory, *, device: int = 0):
    """faiss_index_load_directory: the FaissIvfFlat, FaissIvfPq or FaissOpqIvfPq the directory holds."""
    lib = _lib()
    kind, h = C.c_int32(), C.c_void_p()
    _check(lib, lib.faiss_index_load_directory(device, _path(directory), int(dimension), int(metric), C.byref(kind), C.byref(h)))
    return _FAMILY[kind.value]._from_handle(h)


class FaissIndex:
    """FaissIndex.loadIndex (FaissIndex.scala:28-): dimension and metric come from the caller and must be the file's."""

    @staticmethod
    def load_index(dimension: int, metric: DistanceMetric, directory, *, device: int = 0) -> FaissQueryable:
        return FaissQueryable(load_native_index(dimension, metric, directory, device=device), metric)


# ---- hourly shards ------------------------------------------------------------------------------------------------------
def _utc(t) -> _dt.datetime:
    if isinstance(t, (int, float)):
        return _dt.datetime.fromtimestamp(t, _dt.timezone.utc)
    if t.tzinfo is None:
        return t.replace(tzinfo=_dt.timezone.utc)
    return t.astimezone(_dt.timezone.utc)


def list_hourly_index_directories(root, starting_from, count: int, lookback_interval: int) -> List[str]:
    """HourlyDirectoryWithSuccessFileListing.listHourlyIndexDirectories (:16-63): from starting_from (a UTC datetime, or
    seconds since the epoch) one hour back per step, root/yyyy/MM/dd/HH counts if its _SUCCESS can be read; every step
    costs one of lookback_interval attempts, found or not; at most count directories, newest first."""
    t = _utc(starting_from)
    found: List[str] = []
    attempts = lookback_interval
    while len(found) < count and attempts > 0:
        folder = os.path.join(os.fspath(root), t.strftime("%Y/%m/%d/%H"))
        ok = os.path.join(folder, SUCCESS_FILE_NAME)
        if os.path.isfile(ok) and os.access(ok, os.R_OK):
            found.append(folder)
        t -= _dt.timedelta(hours=1)
        attempts -= 1
    return found


class HourlyShardedIndex:
    """HourlyShardedIndex.scala: the newest shards_to_load hourly directories under root, served as one index.  reload(now)
    is the body of the reference's task() (:66-93); the timer that calls it every shardWatchInterval is the caller's.
    Loaded shards are kept by directory as MemoizedInEpochs keeps them: an unchanged set reloads nothing, a changed one
    reads only the new directories and closes the dropped ones.  search() goes through a ShardSet (shard_set.h) that holds
    the shards being served: the queries go up once, every shard searches them on the device and its answer is folded
    there into the best k by (distance, id); ids pass through as they are and duplicates across shards are kept, as
    IndexShards(d, threaded = false, successive_ids = false) does.  search_composed() is the same answer, byte for byte,
    by the host: every shard's own search, then dann_compose_shards.  FaissQueryable and, with ht,
    polysemous_ann.PolysemousFaissQueryable work over it unchanged."""

    def __init__(self, metric: DistanceMetric, dimension: int, root, shards_to_load: int, lookback_interval: int, *, device: int = 0):
        self.metric, self.dimension, self.root = DistanceMetric(metric), int(dimension), os.fspath(root)
        self.shards_to_load, self.lookback_interval, self.device = int(shards_to_load), int(lookback_interval), device
        self._shards: Dict[str, object] = {}
        self._order: List[str] = []
        self._set: Optional[ShardSet] = None  # made by the first reload that changes the set
        self._started = False  # a reload has found a shard (the reference's castedIndex != null)
        self.loads = 0    # directories read since construction
        self.closes = 0   # shards closed since construction

    @property
    def directories(self) -> List[str]:
        """The directories being served, newest first."""
        return list(self._order)

    def reload(self, now) -> bool:
        """reloadShards() (:66-93): True if the set of shards changed.  As there, only a reload that has never found a
        shard raises; a later one that finds none serves an empty set (every search answers with counts 0).  If a
        directory of a changed set cannot be loaded, the shards loaded for that set are closed again, the error is raised
        and the index goes on serving the set it had."""
        fresh = list_hourly_index_directories(self.root, now, self.shards_to_load, self.lookback_interval)
        changed = set(fresh) != set(self._shards)
        if changed:
            shards, new = {}, []
            try:
                for directory in fresh:
                    if directory in self._shards:
                        shards[directory] = self._shards[directory]
                    else:
                        shards[directory] = load_native_index(self.dimension, self.metric, directory, device=self.device)
                        new.append(shards[directory])
                        self.loads += 1
                if self._set is None:
                    self._set = ShardSet.create(self.metric, self.dimension, device=self.device)
                self._set.set_members([shards[d] for d in fresh])  # (the body of the reference's replaceIndex)
            except Exception:
                for s in new:
                    s.close()
                    self.closes += 1
                raise
            dropped = [s for d, s in self._shards.items() if d not in shards]
            self._shards, self._order = shards, fresh
            self._started = self._started or bool(shards)
            for s in dropped:
                s.close()
                self.closes += 1
        if not self._started:
            raise RuntimeError("requirement failed: Failed to find any shards during startup")
        return changed

    def search(self, queries: np.ndarray, k: int, nprobe: int, ht: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The shards' answers merged on the device (ShardSet.search).  ht > 0 is the Hamming filter of IVF-PQ and OPQ
        shards; IVF-Flat shards refuse it."""
        if not self._started:
            raise RuntimeError("no shard was ever loaded: call reload() first")
        return self._set.search(_rows(queries, self.dimension), k, nprobe, ht)

    def search_composed(self, queries: np.ndarray, k: int, nprobe: int, ht: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """search() by the host: every shard's own search from host memory, merged by dann_compose_shards."""
        if not self._started:
            raise RuntimeError("no shard was ever loaded: call reload() first")
        q = _rows(queries, self.dimension)
        if not self._order:  # an empty IndexShards: nothing to find
            return np.zeros((q.shape[0], k), np.int64), np.zeros((q.shape[0], k), np.float32), np.zeros(q.shape[0], np.int32)
        shards = [self._shards[d] for d in self._order]
        if ht > 0:
            return dense_ann.compose([polysemous_ann.search_ht(s, q, k, nprobe, ht) for s in shards], k)
        return dense_ann.compose([s.search(q, k, nprobe) for s in shards], k)

    def last_stats(self) -> dict:
        """ShardSet.last_stats of the last search(): bus bytes and the search / fold split."""
        if self._set is None:
            raise RuntimeError("no shard was ever loaded: call reload() first")
        return self._set.last_stats()

    def close(self) -> None:
        if self._set is not None:
            self._set.close()
            self._set = None
        for s in self._shards.values():
            s.close()
            self.closes += 1
        self._shards, self._order = {}, []
