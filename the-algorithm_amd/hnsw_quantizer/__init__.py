"""ctypes binding of include/ivf_hnsw_quantizer.h (Faiss `IVF<nlist>_HNSW<M>`): an HNSW graph over the centroids of a
FaissIvfFlat, FaissIvfPq or FaissOpqIvfPq, walked instead of scanned; Faiss's index_factory for those strings, the
reference's index build over it, the queryable that serves FaissRuntimeParam.quantizer_ef, and saving and loading.

Reference (paths relative to the reference's ann/src/main/):
  thrift/com/twitter/ann/common/ann_common.thrift:44-56            FaissRuntimeParam.quantizer_ef
  scala/com/twitter/ann/faiss/FaissIndexer.scala:82-92             index_factory -> train -> add_with_ids
  scala/com/twitter/ann/faiss/QueryableIndexAdapter.scala:70-89    ensuringParams: set_index_parameters under a lock
The quantizer is state of the index it is attached to: every function here takes the index (a refined index stands for its
base) and nothing is added to the index classes.  The default coarse search stays the exhaustive one.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import re
import struct
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .. import binding as _binding
from .. import faiss_files, hnsw_ann, ivfpq_ann, opq_ann, polysemous_ann, refine_ann
from ..dense_ann import DistanceMetric
from ..ivf_ann import MAX_COSINE_DISTANCE, FaissParams, FaissQueryable, IvfError, _rows
from ..simclusters_ann import load_library

_P = C.POINTER
PROTOS = {
    "ivfhq_last_error": (C.c_char_p, []),
    "ivfhq_build": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_int32]),
    "ivfhq_attach_graph": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "ivfhq_detach": (C.c_int, [C.c_int32, C.c_void_p]),
    "ivfhq_set_ef": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32]),
    "ivfhq_info": (C.c_int, [C.c_int32, C.c_void_p, _P(C.c_int32), _P(C.c_int32), _P(C.c_int32)]),
    "ivfhq_quantizer": (C.c_int, [C.c_int32, C.c_void_p, _P(C.c_void_p)]),
    "ivfhq_last_queries": (C.c_int, [C.c_int32, C.c_void_p, _P(C.c_int32), _P(C.c_int32), C.c_void_p]),
    "ivfhq_last_stats": (C.c_int, [C.c_int32, C.c_void_p, _P(C.c_int64), _P(C.c_int64), _P(C.c_int64)]),
}

DEFAULT_QUANTIZER_EF = 16    # Faiss: HNSW::efSearch
DEFAULT_EF_CONSTRUCTION = 40  # Faiss: HNSW::efConstruction
MAX_QUANTIZER_EF = 1024
QUANTIZER_FILE_NAME = "ivf_hnsw_quantizer.bin"


class HnswQuantizerError(IvfError):
    pass


_lib = _binding.binder(PROTOS, "ivfhq", load_library, also=(hnsw_ann._lib,))
_check = _binding.checker(HnswQuantizerError, "ivf_hnsw_quantizer", "ivfhq_last_error")


def _target(index) -> Tuple[int, object]:
    """(FAISS_KIND_*, handle) of the index that holds the quantizer: the index itself, or the base of a refined one."""
    holder = index.base if isinstance(index, refine_ann.FaissRefineFlat) else index
    kind = getattr(holder, "FAISS_KIND", None)
    if kind not in faiss_files._FAMILY:
        raise TypeError(f"{type(index).__name__} is not an inverted-file index (FaissIvfFlat, FaissIvfPq, FaissOpqIvfPq or a "
                        "FaissRefineFlat over one)")
    return kind, holder._h


# ---- the quantizer of an index ------------------------------------------------------------------------------------------
def attach(index, *, max_m: int = 32, ef_construction: int = DEFAULT_EF_CONSTRUCTION, seed: int = 1, batch: int = 0, graph=None) -> None:
    """Builds the graph over the index's stored centroids on the device (deterministic) and attaches it, in place of any
    the index has; quantizer_ef goes back to its default.  graph: attach this one instead, as it stands -- (entry_level,
    entry_item, entry_offsets, entry_neighbours, entry_point, max_level), what hnsw_ann.Hnsw.graph() returns."""
    lib = _lib()
    kind, h = _target(index)
    if graph is None:
        _check(lib, lib.ivfhq_build(kind, h, int(max_m), int(ef_construction), int(seed), int(batch)))
        return
    lv, it, off, nb, entry, max_level = graph
    lv, it = np.ascontiguousarray(lv, np.int32), np.ascontiguousarray(it, np.int64)
    off, nb = np.ascontiguousarray(off, np.int64), np.ascontiguousarray(nb, np.int64)
    if it.shape != lv.shape or off.shape != (lv.shape[0] + 1,):
        raise ValueError("a graph is (entry_level [e], entry_item [e], entry_offsets [e + 1], entry_neighbours, entry_point, max_level)")
    _check(lib, lib.ivfhq_attach_graph(kind, h, int(max_m), int(entry), int(max_level), lv.shape[0], _binding.ptr(lv), _binding.ptr(it),
                                       _binding.ptr(off), _binding.ptr(nb) if nb.size else None))


def detach(index) -> None:
    """Back to the exhaustive coarse search."""
    lib = _lib()
    _check(lib, lib.ivfhq_detach(*_target(index)))


def set_quantizer_ef(index, ef: int) -> None:
    """quantizer_ef in 1..1024, state on the index; refused when no quantizer is attached."""
    lib = _lib()
    _check(lib, lib.ivfhq_set_ef(*_target(index), int(ef)))


def info(index) -> dict:
    """attached, max_m and quantizer_ef of the index."""
    lib = _lib()
    a, m, ef = C.c_int32(), C.c_int32(), C.c_int32()
    _check(lib, lib.ivfhq_info(*_target(index), C.byref(a), C.byref(m), C.byref(ef)))
    return {"attached": bool(a.value), "max_m": m.value, "quantizer_ef": ef.value}


def quantizer(index) -> Optional[hnsw_ann.Hnsw]:
    """The graph as an hnsw_ann.Hnsw over the borrowed handle (None: no quantizer): its exports and its search work, its
    close() does nothing, and it must not be appended to or updated.  It goes with the index, or with the next attach or
    detach."""
    lib = _lib()
    kind, h = _target(index)
    g = C.c_void_p()
    _check(lib, lib.ivfhq_quantizer(kind, h, C.byref(g)))
    if not g.value:
        return None
    n, d, metric, max_m = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
    hnsw_ann._check(lib, lib.hnsw_index_info(g, C.byref(n), C.byref(d), C.byref(metric), C.byref(max_m)))
    view = hnsw_ann.Hnsw(g, DistanceMetric(metric.value), n.value, d.value, max_m.value)
    view._owned = False  # borrowed: the index destroys it
    return view


def last_queries(index) -> np.ndarray:
    """The prepared queries the last search walked: fp32 [nq, d] holding fp16 values (Cosine: unit length)."""
    lib = _lib()
    kind, h = _target(index)
    nq, d = C.c_int32(), C.c_int32()
    _check(lib, lib.ivfhq_last_queries(kind, h, C.byref(nq), C.byref(d), None))
    out = np.empty((nq.value, d.value), np.float32)
    if nq.value:
        _check(lib, lib.ivfhq_last_queries(kind, h, None, None, out.ctypes.data))
    return out


def last_quantizer_stats(index) -> dict:
    """The walks of the last search: distance_evals, expansions, missing_probes."""
    lib = _lib()
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    _check(lib, lib.ivfhq_last_stats(*_target(index), C.byref(a), C.byref(b), C.byref(c)))
    return {"distance_evals": a.value, "expansions": b.value, "missing_probes": c.value}


# ---- index_factory and the reference's build ----------------------------------------------------------------------------
_HNSW = re.compile(r"((?:.*,)?IVF\d+)_HNSW(\d+)(,.*)")
_REFINE = re.compile(r".*,(?:RFlat|Refine\(Flat\))")


def _inner_factory(dimension: int, factory_string, metric: DistanceMetric):
    """The outermost of the older factories that serves the string."""
    if isinstance(factory_string, str):
        if _REFINE.fullmatch(factory_string):
            return refine_ann.index_factory(dimension, factory_string, metric)
        if factory_string.endswith("np"):
            return polysemous_ann.index_factory(dimension, factory_string, metric)
        if factory_string.startswith("OPQ"):
            return opq_ann.index_factory(dimension, factory_string, metric)
    return ivfpq_ann.index_factory(dimension, factory_string, metric)


class HnswQuantizedIndexSpec:
    """What index_factory returns for an `IVF<nlist>_HNSW<M>` string: an untrained index.  train() trains the inner spec
    as it always trains (k-means against the exhaustive search), then builds the graph over the final centroids; a
    refined index is wrapped after that, so that it inherits the quantizer."""

    def __init__(self, inner_spec, max_m: int, factory_string: str):
        self.inner_spec, self.max_m, self.factory_string = inner_spec, int(max_m), factory_string
        self.dimension, self.metric = inner_spec.dimension, inner_spec.metric

    @property
    def index_class(self):
        return self.inner_spec.index_class

    def train(self, vectors: np.ndarray, niter: int = 0, seed: int = 1, *, ef_construction: int = DEFAULT_EF_CONSTRUCTION,
              quantizer_seed: int = 1, **kwargs):
        refined = isinstance(self.inner_spec, refine_ann.RefineIndexSpec)
        base_spec = self.inner_spec.base_spec if refined else self.inner_spec
        index = base_spec.train(vectors, niter, seed, **kwargs)
        try:
            attach(index, max_m=self.max_m, ef_construction=ef_construction, seed=quantizer_seed)
            return refine_ann.FaissRefineFlat.wrap(index, self.inner_spec.k_factor) if refined else index
        except Exception:
            index.close()
            raise


def index_factory(dimension: int, factory_string: str, metric: DistanceMetric):
    """Faiss's index_factory for `IVF<nlist>_HNSW<M>` where Faiss accepts it: `IVF<nlist>_HNSW<M>,Flat`,
    `IVF<nlist>_HNSW<M>,PQ<M>[x8]`, the latter behind `OPQ<M>[_<dout>],` and in front of `,RFlat`.  The string without
    `_HNSW<M>` goes to refine_ann, polysemous_ann, opq_ann or ivfpq_ann, whichever is outermost, whose refusals are this
    one's.  A string without `_HNSW` goes straight through, unchanged."""
    if not isinstance(factory_string, str) or "_HNSW" not in factory_string:
        return _inner_factory(dimension, factory_string, metric)
    m = _HNSW.fullmatch(factory_string)
    if m is None:
        raise ValueError(f"index_factory: unsupported factory string {factory_string!r} (the HNSW coarse quantizer is written "
                         "IVF<nlist>_HNSW<M>, in front of ,Flat or ,PQ<M>)")
    max_m = int(m.group(2))
    if not 2 <= max_m <= 32:
        raise ValueError(f"index_factory: {factory_string!r}: HNSW{max_m}: the graph's M must be in 2..32")
    try:
        inner = _inner_factory(dimension, m.group(1) + m.group(3), metric)
    except ValueError as e:
        raise ValueError(f"index_factory: {factory_string!r}: without its quantizer the string is refused: {e}") from None
    return HnswQuantizedIndexSpec(inner, max_m, factory_string)


def build_faiss_index(vectors: np.ndarray, ids: Sequence[int], sample_rate: float, factory_string: str,
                      metric: DistanceMetric = DistanceMetric.Cosine, *, ef_construction: int = DEFAULT_EF_CONSTRUCTION,
                      quantizer_seed: int = 1, niter: int = 0, seed: int = 1, device: int = 0, **kwargs):
    """FaissIndexer.buildAndWriteFaissIndex (:82-92) without the write, over this module's index_factory: train on the
    first trainingSetSize rows, build the quantizer over the trained centroids, then add_with_ids all rows -- through the
    quantizer, as Faiss adds.  The graph's M comes from the string.  kwargs: what the inner spec's train() takes
    (niter_opq, anneal_iters)."""
    v = _rows(vectors)
    spec = index_factory(v.shape[1], factory_string, metric)
    head = v[:ivfpq_ann.training_set_size(v.shape[0], sample_rate)]
    if isinstance(spec, HnswQuantizedIndexSpec):
        index = spec.train(head, niter, seed, ef_construction=ef_construction, quantizer_seed=quantizer_seed, device=device, **kwargs)
    else:
        index = spec.train(head, niter, seed, device=device, **kwargs)
    index.add(v, ids)
    return index


# ---- the queryable ------------------------------------------------------------------------------------------------------
class HnswQuantizedFaissQueryable(FaissQueryable):
    """FaissQueryable over an index with an HNSW quantizer: FaissParams.quantizerEf is set on the index before the search
    (None leaves it as it is), nprobe and ht are served as PolysemousFaissQueryable serves them (ht only by an index with
    product-quantiser codes); quantizerKfactorRf and quantizerNprobe stay refused.  One query at a time per index: the
    parameter is state of the index, as in the reference."""

    @staticmethod
    def _params(params: FaissParams) -> Tuple[int, Optional[int], Optional[int]]:
        others = [f for f in ("quantizerKfactorRf", "quantizerNprobe") if getattr(params, f) is not None]
        if others:
            raise ValueError("the coarse quantizer of this index is an HNSW graph, with no refinement and no inner nprobe to "
                             "tune: " + ", ".join(others) + " cannot be set (only nprobe, quantizerEf and ht)")
        if params.nprobe is None:
            raise ValueError("FaissParams.nprobe must be set")
        return (int(params.nprobe), None if params.quantizerEf is None else int(params.quantizerEf),
                None if params.ht is None else int(params.ht))

    def queryWithDistance(self, embedding: np.ndarray, numOfNeighbors: int, runtimeParams: FaissParams) -> List[Tuple[int, float]]:
        nprobe, ef, ht = self._params(runtimeParams)
        if ef is not None:
            set_quantizer_ef(self.index, ef)
        q = np.asarray(embedding, np.float32)
        if ht is None:
            ids, dist, cnt = self.index.search(q, numOfNeighbors, nprobe)
        elif isinstance(self.index, polysemous_ann._HtSearch):
            ids, dist, cnt = self.index.search(q, numOfNeighbors, nprobe, ht)
        else:
            ids, dist, cnt = polysemous_ann.search_ht(self.index, q, numOfNeighbors, nprobe, ht)
        m = int(cnt[0])
        out_d = np.array(dist[0, :m], np.float32)
        if self.metric == DistanceMetric.Cosine:
            sim = np.float32(1.0) - out_d
            out_d = np.where((sim < 0) | (sim > 1), np.float32(MAX_COSINE_DISTANCE), out_d).astype(np.float32)
        return list(zip(np.asarray(ids[0, :m]).tolist(), out_d.tolist()))


# ---- saving and loading -------------------------------------------------------------------------------------------------
# The quantizer file, beside the unchanged faiss.index: a header of little-endian int64 (magic, version, nlist, max_m,
# entry_point, max_level, n_entries, n_neighbours), entry_level int32 [e], entry_item int64 [e], entry_offsets int64 [e + 1],
# entry_neighbours int64 [nn], then the SHA-256 of everything before it.
_MAGIC, _VERSION, _HEADER = 0x51484E5746564949, 1, struct.Struct("<8q")
MAX_GRAPH_LEVEL = 64


class QuantizerFileError(HnswQuantizerError):
    pass


def encode_quantizer(nlist: int, max_m: int, graph) -> bytes:
    lv, it, off, nb, entry, max_level = graph
    lv, it = np.ascontiguousarray(lv, "<i4"), np.ascontiguousarray(it, "<i8")
    off, nb = np.ascontiguousarray(off, "<i8"), np.ascontiguousarray(nb, "<i8")
    body = _HEADER.pack(_MAGIC, _VERSION, int(nlist), int(max_m), int(entry), int(max_level), lv.shape[0], nb.shape[0])
    body += lv.tobytes() + it.tobytes() + off.tobytes() + nb.tobytes()
    return body + hashlib.sha256(body).digest()


def decode_quantizer(data: bytes, nlist: Optional[int] = None):
    """(max_m, graph) of a quantizer file's bytes, every count and index checked before anything is built from it; a file
    cut short, grown or changed in any bit is refused.  nlist: what the index beside it has."""
    def refuse(why):
        return QuantizerFileError(f"quantizer file refused: {why}")

    if len(data) < _HEADER.size + 32:
        raise refuse(f"{len(data)} bytes are fewer than its header and checksum")
    body, digest = data[:-32], data[-32:]
    if hashlib.sha256(body).digest() != digest:
        raise refuse("the checksum does not match: the file is truncated or corrupted")
    magic, version, f_nlist, max_m, entry, max_level, ne, nn = _HEADER.unpack_from(body)
    if magic != _MAGIC or version != _VERSION:
        raise refuse("not a quantizer file of this version")
    if not 1 <= f_nlist <= 65536 or (nlist is not None and f_nlist != nlist):
        raise refuse(f"it is a graph over {f_nlist} cells" + ("" if nlist is None else f", the index has {nlist}"))
    if not 2 <= max_m <= 32 or not 0 <= entry < f_nlist or not 0 <= max_level <= MAX_GRAPH_LEVEL:
        raise refuse("max_m, entry point or max level out of range")
    if not 0 <= ne <= f_nlist * (MAX_GRAPH_LEVEL + 1) or not 0 <= nn <= ne * 2 * max_m:
        raise refuse("entry or neighbour count out of range")
    if len(body) != _HEADER.size + ne * 4 + ne * 8 + (ne + 1) * 8 + nn * 8:
        raise refuse("its length does not fit its counts")
    at = _HEADER.size
    lv = np.frombuffer(body, "<i4", ne, at).astype(np.int32); at += ne * 4
    it = np.frombuffer(body, "<i8", ne, at).astype(np.int64); at += ne * 8
    off = np.frombuffer(body, "<i8", ne + 1, at).astype(np.int64); at += (ne + 1) * 8
    nb = np.frombuffer(body, "<i8", nn, at).astype(np.int64)
    if ne and (lv.min() < 0 or lv.max() > max_level or it.min() < 0 or it.max() >= f_nlist):
        raise refuse("an entry's level or item is out of range")
    if off[0] != 0 or off[-1] != nn or (np.diff(off) < 0).any():
        raise refuse("the entry offsets do not partition the neighbours")
    if nn and (nb.min() < 0 or nb.max() >= f_nlist):
        raise refuse("a neighbour is outside [0, nlist)")
    return int(max_m), (lv, it, off, nb, int(entry), int(max_level))


def write_index(index, directory) -> None:
    """faiss_files.write_index with the quantizer beside it: the unchanged faiss.index through the existing writer, then the
    graph in QUANTIZER_FILE_NAME (under a temporary name, renamed), and _SUCCESS last.  The old loader reads the same
    directory as an exhaustive index.  Without a quantizer it is faiss_files.write_index."""
    view = quantizer(index)
    if view is None:
        faiss_files.write_index(index, directory)
        return
    directory = os.fspath(directory)
    data = encode_quantizer(index.nlist, view.max_m, view.graph())
    faiss_files.write_index(index, directory)
    # the existing writer ends with _SUCCESS: it comes away until the quantizer file is in, so that it stays the last
    success = os.path.join(directory, faiss_files.SUCCESS_FILE_NAME)
    os.remove(success)
    tmp = os.path.join(directory, QUANTIZER_FILE_NAME + ".tmp")
    with open(tmp, "wb") as f:
        f.write(data)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, os.path.join(directory, QUANTIZER_FILE_NAME))
    with open(success, "wb"):
        pass


def load_index(dimension: int, metric: DistanceMetric, directory, *, device: int = 0):
    """The index of the directory with its quantizer attached, the graph entry for entry as saved; quantizer_ef is back at
    its default.  The quantizer file is read and checked before any device work; a directory without one gives the plain
    index."""
    path = os.path.join(os.fspath(directory), QUANTIZER_FILE_NAME)
    data = None
    if os.path.exists(path):
        with open(path, "rb") as f:
            data = f.read()
        decode_quantizer(data)
    index = faiss_files.load_native_index(dimension, metric, directory, device=device)
    if data is None:
        return index
    try:
        max_m, graph = decode_quantizer(data, nlist=index.nlist)
        attach(index, max_m=max_m, graph=graph)
        return index
    except Exception:
        index.close()
        raise
