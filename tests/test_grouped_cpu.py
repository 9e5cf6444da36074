"""The grouped index (include/grouped_ann.h) without a GPU: the exported symbols, argument errors that return before any
device call, the key table and group_rows of the Python mirror, and the CPU restatement tests/_grouped_ref.py against
hand-derived answers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _grouped_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1


def test_library_exports_every_declared_symbol(pkg):
    lib = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "grouped_ann.h")).read()
    declared = set(re.findall(r"\b(gann_[a-z_0-9]+)\s*\(", header))
    assert len(declared) >= 7, "declarations parsed"
    assert declared == set(pkg.grouped_ann.PROTOS)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/grouped_ann.h but not exported"


def test_status_codes_carry_the_numbers_of_ivf_ann():
    def defines(name, prefix):
        text = open(os.path.join(ROOT, "include", name)).read()
        return {m[0]: int(m[1]) for m in re.findall(r"#define %s_([A-Z_]+) (\d+)" % prefix, text)}

    assert defines("grouped_ann.h", "GANN") == defines("ivf_ann.h", "IVF")


def test_argument_errors_return_before_any_device_call(pkg):
    lib = pkg.grouped_ann._lib()
    h = C.c_void_p()
    x = np.zeros((8, 32), np.float32)
    g = np.zeros(8, np.int32)

    def err():
        return lib.gann_last_error().decode()

    def build(metric=0, d=32, n_groups=4, n=8, vectors=x.ctypes.data, groups=g.ctypes.data, out=C.byref(h)):
        return lib.gann_index_build(0, metric, d, n_groups, n, vectors, None, groups, out)

    assert build(vectors=None) == EINVAL and "null" in err()
    assert build(groups=None) == EINVAL and "null" in err()
    assert build(out=None) == EINVAL and "null" in err()
    for d in (8, 24, 528):
        assert build(d=d) == EINVAL and "multiple of 16" in err()
    for n_groups in (0, 1048577):
        assert build(n_groups=n_groups) == EINVAL and "n_groups" in err()
    assert build(metric=7) == EINVAL and "metric" in err()
    assert build(n=-1) == EINVAL
    assert build(n=2 ** 31 - 64) == EINVAL
    for bad in (-1, 4):
        g[:] = [0, 3, 1, 2, 3, bad, bad, 0]
        assert build() == EINVAL and "row 5" in err() and str(bad) in err()
    g[:] = 0
    assert h.value is None

    out = np.zeros(2048, np.int64)
    o = out.ctypes.data

    def search(ix, nq=1, queries=x.ctypes.data, groups=g.ctypes.data, k=1, od=o, oi=o, oc=o):
        return lib.gann_search(ix, nq, queries, groups, k, od, oi, oc)

    # k and nq are refused before the handle is looked at: any non-NULL pointer will do
    fake = C.create_string_buffer(4096)
    addr = C.addressof(fake)
    assert search(None) == EINVAL and "null" in err()
    assert search(addr, queries=None) == EINVAL and "null" in err()
    assert search(addr, groups=None) == EINVAL and "null" in err()
    assert search(addr, od=None) == EINVAL and search(addr, oi=None) == EINVAL and search(addr, oc=None) == EINVAL
    for k in (0, 1025):
        assert search(addr, k=k) == EINVAL and "k must" in err()
    assert search(addr, nq=0) == EINVAL and "nq" in err()
    assert lib.gann_index_info(None, None, None, None, None) == EINVAL
    assert lib.gann_index_group_sizes(None, o) == EINVAL
    assert lib.gann_last_stats(None, None, None, None, None, None, None, None, None) == EINVAL
    assert lib.gann_index_destroy(None) == 0


def test_key_table_and_group_rows(pkg):
    ga = pkg.grouped_ann
    table, groups = ga.key_table(["fr", "en", "fr", "", "ja", "en"])
    assert table == ["fr", "en", "", "ja"], "first-appearance order"
    assert groups.dtype == np.int32 and groups.tolist() == [0, 1, 0, 2, 3, 1]
    ix = ga.GroupedIndex(None, pkg.dense_ann.DistanceMetric.L2, 16, table)
    assert ix.group_numbers(["ja", None, "de", "", "fr"]).tolist() == [3, -1, -1, 2, 0], "None and unknown keys are -1"

    emb = [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0]]
    got = ga.group_rows([7, None, 9, 8], emb, ["b", "a", "a", "b"])
    assert list(got) == ["b", "a"], "first-appearance order; the row without an entity id is dropped"
    assert [i for i, _ in got["b"]] == [7, 8] and [i for i, _ in got["a"]] == [9]
    assert got["b"][1][1].dtype == np.float32 and got["b"][1][1].tolist() == [7.0, 8.0]
    flat = ga.group_rows([1, 2, 3, 4], emb)
    assert list(flat) == [""] and [i for i, _ in flat[""]] == [1, 2, 3, 4], "flat data is the single key ''"
    with pytest.raises(ValueError):
        ga.group_rows([1, 2], emb)


def _axis(*pairs):
    v = np.zeros(16, np.float32)
    for k, a in pairs:
        v[k] = a
    return v


# seven rows in three groups of a four-group index (every value exact in fp16); group 3 stays empty
ROWS = np.stack([
    _axis((0, 1.0)),             # id 10  group 0
    _axis((0, 1.0)),             # id 5   group 0, a duplicate of id 10
    _axis((1, 1.0)),             # id 20  group 1
    _axis((0, 0.75), (1, 0.25)), # id 7   group 0
    _axis((0, 1.0), (1, 0.5)),   # id 21  group 1: the query itself
    _axis((0, 0.5), (1, 0.5)),   # id 1   group 0
    _axis((0, 0.25)),            # id 30  group 2
])
IDS = np.array([10, 5, 20, 7, 21, 1, 30], np.int64)
GROUPS = [0, 0, 1, 0, 1, 0, 2]
Q = _axis((0, 1.0), (1, 0.5))


def test_reference_answers_by_hand():
    q = np.stack([Q] * 6)
    qg = [0, 1, 2, 3, -1, 4]
    ix = ref.GroupedRef(ref.INNER_PRODUCT, 4, ROWS, IDS, GROUPS)
    assert ix.group_sizes().tolist() == [4, 2, 1, 0]
    res = ix.search(q, qg, 3)
    # group 0: dots 1, 1, 0.875, 0.75 for ids 10, 5, 7, 1 -> the tie goes to the lower id; id 21 (dot 1.25) is not in it
    assert res[0][0].tolist() == [5, 10, 7] and res[0][1].tolist() == [0.0, 0.0, 0.125] and res[0][2] == 0.25
    # group 1: dots 1.25 and 0.5
    assert res[1][0].tolist() == [21, 20] and res[1][1].tolist() == [-0.25, 0.5] and res[1][2] == np.inf
    assert res[2][0].tolist() == [30] and res[2][1].tolist() == [0.75]
    for r in res[3:]:
        assert len(r[0]) == 0 and len(r[1]) == 0, "the empty group and the groups outside the index answer nothing"
    # L2, group 0: id 7 at sqrt(1/8), then ids 1, 5, 10 all at 0.5
    ix = ref.GroupedRef(ref.L2, 4, ROWS, IDS, GROUPS)
    res = ix.search(q[:2], qg[:2], 3)
    assert res[0][0].tolist() == [7, 1, 5]
    np.testing.assert_allclose(res[0][1], [np.sqrt(0.125), 0.5, 0.5], rtol=1e-12)
    assert res[0][2] == 0.5
    assert res[1][0].tolist() == [21, 20] and res[1][1][0] == 0.0
    # ids = None: positions
    ix = ref.GroupedRef(ref.INNER_PRODUCT, 4, ROWS, None, GROUPS)
    assert ix.search(q[:1], [0], 4)[0][0].tolist() == [0, 1, 3, 5]
    with pytest.raises(ValueError, match="row 2"):
        ref.GroupedRef(ref.L2, 4, ROWS, IDS, [0, 0, 4, 0, 1, 0, 2])
