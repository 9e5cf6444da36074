"""The HNSW coarse quantizer of the IVF family (include/ivf_hnsw_quantizer.h) without a GPU: the exported symbols, the
argument refusals that come before any device call, index_factory, the queryable over a stub, and the quantizer file."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import _ivfhq_ref as hqref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1


@pytest.fixture(scope="module")
def hq(pkg):
    return importlib.import_module(pkg.__name__ + ".hnsw_quantizer")


def test_library_exports_every_declared_symbol(pkg, hq):
    lib = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "ivf_hnsw_quantizer.h")).read()
    declared = set(re.findall(r"\b(ivfhq_[a-z_0-9]+)\s*\(", header))
    assert len(declared) == 9, "declarations parsed"
    assert declared == set(hq.PROTOS)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/ivf_hnsw_quantizer.h but not exported"


def test_package_does_not_reexport_the_subpackage_names(pkg, hq):
    for name in ("HnswQuantizedFaissQueryable", "set_quantizer_ef", "attach", "detach", "quantizer"):
        assert not hasattr(pkg, name)


def test_argument_errors_return_before_any_device_call(hq):
    lib = hq._lib()

    def err():
        return lib.ivfhq_last_error().decode()

    fake = C.create_string_buffer(4096)
    addr = C.addressof(fake)
    i32, i64, p = C.c_int32(), C.c_int64(), C.c_void_p()
    z = np.zeros(4, np.int64)
    calls = {
        "build": lambda kind, h: lib.ivfhq_build(kind, h, 8, 40, 1, 0),
        "attach_graph": lambda kind, h: lib.ivfhq_attach_graph(kind, h, 8, 0, 0, 0, None, None, z.ctypes.data, None),
        "detach": lambda kind, h: lib.ivfhq_detach(kind, h),
        "set_ef": lambda kind, h: lib.ivfhq_set_ef(kind, h, 16),
        "info": lambda kind, h: lib.ivfhq_info(kind, h, C.byref(i32), C.byref(i32), C.byref(i32)),
        "quantizer": lambda kind, h: lib.ivfhq_quantizer(kind, h, C.byref(p)),
        "last_queries": lambda kind, h: lib.ivfhq_last_queries(kind, h, C.byref(i32), C.byref(i32), None),
        "last_stats": lambda kind, h: lib.ivfhq_last_stats(kind, h, C.byref(i64), C.byref(i64), C.byref(i64)),
    }
    for name, call in calls.items():
        for kind in (1, 2, 3):
            assert call(kind, None) == EINVAL and "null" in err(), name
        # the kind is looked at before the handle is: any non-NULL pointer will do
        for kind in (0, 4, -1):
            assert call(kind, addr) == EINVAL and "kind" in err(), name
    assert p.value is None
    # quantizer_ef is refused before the handle is looked at
    for ef in (0, 1025, -3):
        assert lib.ivfhq_set_ef(1, addr, ef) == EINVAL and "quantizer_ef" in err()
        assert lib.ivfhq_set_ef(1, None, ef) == EINVAL
    with pytest.raises(TypeError, match="inverted-file"):
        hq.set_quantizer_ef(object(), 16)


@pytest.mark.parametrize("string, max_m, inner, inner_string", [
    ("IVF64_HNSW32,Flat", 32, "IndexSpec", "IVF64,Flat"),
    ("IVF64_HNSW8,PQ8", 8, "IndexSpec", "IVF64,PQ8"),
    ("OPQ16,IVF64_HNSW32,PQ16", 32, "OpqIndexSpec", "OPQ16,IVF64,PQ16"),
    ("IVF64_HNSW32,PQ8,RFlat", 32, "RefineIndexSpec", "IVF64,PQ8,RFlat"),
])
def test_index_factory_carries_max_m_and_the_inner_spec(pkg, hq, string, max_m, inner, inner_string):
    metric = pkg.dense_ann.DistanceMetric.L2
    spec = hq.index_factory(64, string, metric)
    assert isinstance(spec, hq.HnswQuantizedIndexSpec)
    assert spec.max_m == max_m and spec.factory_string == string and spec.dimension == 64 and spec.metric == metric
    assert type(spec.inner_spec).__name__ == inner and spec.inner_spec.factory_string == inner_string
    base = spec.inner_spec.base_spec if inner == "RefineIndexSpec" else spec.inner_spec
    assert base.nlist == 64
    if inner == "IndexSpec":
        assert base.M == (None if string.endswith("Flat") else 8)


def test_index_factory_passes_other_strings_through_unchanged(pkg, hq):
    metric = pkg.dense_ann.DistanceMetric.Cosine
    for string, module in (("IVF64,Flat", "ivfpq_ann"), ("IVF64,PQ8", "ivfpq_ann"), ("OPQ16,IVF64,PQ16", "opq_ann"),
                           ("IVF64,PQ8,RFlat", "refine_ann"), ("IVF64,PQ8np", "polysemous_ann")):
        got = hq.index_factory(64, string, metric)
        want = getattr(pkg, module).index_factory(64, string, metric)
        assert type(got) is type(want) and vars(got).keys() == vars(want).keys() and got.factory_string == string


@pytest.mark.parametrize("string", ["IVF64_HNSW,PQ8", "IVF64_HNSW0,PQ8", "IVF64_hnsw32,PQ8", "HNSW32", "IVF64_HNSW33,PQ8",
                                    "IVF64_HNSW32", "IVF64_HNSW32,SQ8", "OPQ16,IVF64_HNSW32,PQ8"])
def test_index_factory_refuses_and_names_the_string(pkg, hq, string):
    with pytest.raises(ValueError, match=re.escape(repr(string))):
        hq.index_factory(64, string, pkg.dense_ann.DistanceMetric.L2)


def test_older_factories_still_refuse_the_quantizer(pkg):
    with pytest.raises(ValueError):
        pkg.ivfpq_ann.index_factory(64, "IVF64_HNSW32,PQ8", pkg.dense_ann.DistanceMetric.L2)


class _Stub:
    def __init__(self, log):
        self.log = log

    def search(self, q, k, nprobe, *ht):
        self.log.append(("search", k, nprobe) + ht)
        return np.arange(100, 103)[None, :], np.array([[-0.25, 0.25, 1.5]], np.float32), np.array([3], np.int32)


def test_queryable_sets_quantizer_ef_before_the_search(pkg, hq, monkeypatch):
    iv, m = pkg.ivf_ann, pkg.dense_ann.DistanceMetric
    log = []
    stub = _Stub(log)
    monkeypatch.setattr(hq, "set_quantizer_ef", lambda index, ef: log.append(("ef", index, ef)))
    qa = hq.HnswQuantizedFaissQueryable(stub, m.Cosine)
    got = qa.queryWithDistance(np.zeros(16), 3, iv.FaissParams(nprobe=5, quantizerEf=7))
    assert log == [("ef", stub, 7), ("search", 3, 5)], "the setter once, then the search"
    assert got == [(100, 1.0), (101, 0.25), (102, 1.0)], "the Cosine translation of FaissQueryable"
    del log[:]
    assert qa.query(np.zeros(16), 3, iv.FaissParams(nprobe=2)) == [100, 101, 102]
    assert log == [("search", 3, 2)], "quantizerEf = None leaves the index as it is"
    for field in ("quantizerKfactorRf", "quantizerNprobe"):
        del log[:]
        with pytest.raises(ValueError, match=field):
            qa.queryWithDistance(np.zeros(16), 3, iv.FaissParams(nprobe=1, quantizerEf=4, **{field: 2}))
        assert log == [], "refused before the setter and the search"
    with pytest.raises(ValueError, match="nprobe"):
        qa.queryWithDistance(np.zeros(16), 3, iv.FaissParams(quantizerEf=4))
    # the plain queryables keep refusing the field
    with pytest.raises(ValueError, match="quantizerEf"):
        iv.FaissQueryable(stub, m.L2).queryWithDistance(np.zeros(16), 3, iv.FaissParams(nprobe=1, quantizerEf=4))
    with pytest.raises(ValueError, match="quantizerEf"):
        pkg.polysemous_ann.PolysemousFaissQueryable(stub, m.L2).queryWithDistance(np.zeros(16), 3, iv.FaissParams(nprobe=1, quantizerEf=4))


def test_queryable_passes_ht_to_an_index_that_filters(pkg, hq):
    class Ht(_Stub, pkg.polysemous_ann._HtSearch):
        pass

    log = []
    qa = hq.HnswQuantizedFaissQueryable(Ht(log), pkg.dense_ann.DistanceMetric.L2)
    qa.queryWithDistance(np.zeros(16), 3, pkg.ivf_ann.FaissParams(nprobe=4, ht=9))
    assert log == [("search", 3, 4, 9)]


_rings = hqref.two_rings  # two rings of four over eight cells, level 0 only


def test_quantizer_file_round_trip(hq):
    data = hq.encode_quantizer(8, 2, _rings())
    max_m, graph = hq.decode_quantizer(data, nlist=8)
    assert max_m == 2 and graph[4:] == (0, 0)
    for got, want in zip(graph[:4], _rings()[:4]):
        assert got.dtype == want.dtype and got.tolist() == want.tolist()


def test_hostile_quantizer_files_are_refused_without_a_device(hq, tmp_path, monkeypatch):
    good = hq.encode_quantizer(8, 2, _rings())
    for cut in (0, 1, 63, 64, 95, len(good) // 2, len(good) - 33, len(good) - 1):
        with pytest.raises(hq.QuantizerFileError):
            hq.decode_quantizer(good[:cut])
    with pytest.raises(hq.QuantizerFileError):
        hq.decode_quantizer(good + b"\0")
    for byte in (0, 8, 17, 40, 64, 70, len(good) - 40, len(good) - 1):
        for bit in (0, 7):
            bad = bytearray(good)
            bad[byte] ^= 1 << bit
            with pytest.raises(hq.QuantizerFileError, match="checksum"):
                hq.decode_quantizer(bytes(bad))
    with pytest.raises(hq.QuantizerFileError, match="cells"):
        hq.decode_quantizer(good, nlist=9)
    # well-formed files whose contents are out of range: the checksum holds, the checks do not
    lv, it, off, nb, entry, ml = _rings()
    hostile = {
        "entry point": (lv, it, off, nb, 8, 0),
        "item": (lv, np.where(it == 3, 8, it), off, nb, 0, 0),
        "neighbour": (lv, it, off, np.where(nb == 5, -1, nb), 0, 0),
        "level": (np.where(it == 2, 1, lv).astype(np.int32), it, off, nb, 0, 0),
        "offsets": (lv, it, off[::-1].copy(), nb, 0, 0),
        "offsets end": (lv, it, off + 1, nb, 0, 0),
        "max level": (lv, it, off, nb, 0, 65),
    }
    for name, graph in hostile.items():
        with pytest.raises(hq.QuantizerFileError):
            hq.decode_quantizer(hq.encode_quantizer(8, 2, graph))
    with pytest.raises(hq.QuantizerFileError):
        hq.decode_quantizer(hq.encode_quantizer(8, 33, _rings()))
    with pytest.raises(hq.QuantizerFileError):
        hq.decode_quantizer(hq.encode_quantizer(0, 2, _rings()))

    # load_index reads and checks the file before it touches the index file or a device
    def no_device(*a, **k):
        raise AssertionError("the index was loaded before the quantizer file was checked")

    monkeypatch.setattr(hq.faiss_files, "load_native_index", no_device)
    for name, data in (("truncated", good[:-5]), ("flipped", bytes(bytearray(good[:70]) + bytes([good[70] ^ 4]) + good[71:]))):
        d = tmp_path / name
        d.mkdir()
        (d / hq.QUANTIZER_FILE_NAME).write_bytes(data)
        with pytest.raises(hq.QuantizerFileError):
            hq.load_index(16, 0, d)
