"""The Annoy index (include/annoy_ann.h) without a GPU: the exported symbols, the forest builder's structure, splits and
determinism, the loader's refusals, limits refused before any device call, neighboursToRequest against the Scala, the CPU
restatement tests/_annoy_ref.py on a forest small enough to follow by hand, and the host code under the sanitizers."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _annoy_ref as ref
from _pkg import ROOT, load_package

pkg = load_package()
an = pkg.annoy_ann
L2, COSINE, IP = 0, 1, 2
EINVAL, ELIMIT = 1, 3
N = 600


def _rows(d, seed=3, n=N):
    rng = np.random.default_rng(seed)
    basis = rng.standard_normal((3, d)) / np.sqrt(3)
    return (rng.standard_normal((n, 3)) @ basis + 0.3 * rng.standard_normal((n, d))).astype(np.float32)


def _flat(f):
    return f.nodes, f.normals.view(np.uint16), f.offsets.view(np.uint32), f.roots, f.items


def _same(f, g):
    return all(np.array_equal(a, b) for a, b in zip(_flat(f), _flat(g)))


def test_every_declared_symbol_is_exported():
    header = open(os.path.join(ROOT, "include", "annoy_ann.h")).read()
    declared = set(re.findall(r"\b(annoy_[a-z_0-9]+)\s*\(", header))
    assert len(declared) >= 20
    assert declared == set(an.PROTOS)
    lib = pkg.load_library()
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/annoy_ann.h but not exported"


def test_prepare_is_the_inverted_file_preparation():
    """annoy_prepare_rows against tests/_ivf_ref.prepare (the statement of ivf_ann.h), and its fp16 rounding against numpy's
    over values that cover subnormal halves, ties and the overflow edge."""
    rng = np.random.default_rng(0)
    x = _rows(100)
    for metric in (L2, COSINE):
        assert np.array_equal(an.prepare(metric, x).astype(np.float32), ref.prepare(metric, x))
    v = np.concatenate([rng.standard_normal(4000) * 10.0 ** rng.integers(-9, 5, 4000), np.arange(2048, 2300) * 2.0 ** -25,
                        [65504, 65519.99, -65504, 0.0, -0.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001, 1 + 2.0 ** -11,
                         1 + 3 * 2.0 ** -11]]).astype(np.float32)
    v = v[np.abs(v) < 65520][:, None]  # rows of one component
    with np.errstate(over="ignore"):
        assert np.array_equal(an.prepare(L2, v).view(np.uint16), v.astype(np.float16).view(np.uint16))
    assert np.all(an.prepare(COSINE, np.zeros((2, 5), np.float32)) == 0)
    with pytest.raises(an.AnnoyError, match="finite"):
        an.prepare(L2, np.array([[1.0, np.inf]], np.float32))


@pytest.mark.parametrize("leaf_size", [2, 0])
@pytest.mark.parametrize("n_trees", [1, 7])
@pytest.mark.parametrize("metric", [L2, COSINE])
@pytest.mark.parametrize("d", [3, 64, 100])
def test_forest_structure_and_splits(d, metric, n_trees, leaf_size):
    x = _rows(d)
    f = an.AnnoyForest.build(metric, x, n_trees, leaf_size, seed=5, threads=2)
    info = f.info()
    leaf = leaf_size or d + 2
    assert info["leaf_size"] == leaf and info["n"] == N and info["n_trees"] == n_trees and info["n_items"] == n_trees * N
    nodes, normals, offsets, roots, items = f.nodes, f.normals, f.offsets, f.roots, f.items
    rows = ref.pad8(an.prepare(metric, x).astype(np.float32))
    sn = ref.split_numbers(nodes)
    assert (nodes[:, 0] == ref.SPLIT).sum() == info["n_splits"] == len(offsets)
    if metric == COSINE:
        assert not offsets.any()
    reached = np.zeros(len(nodes), int)
    for t in range(n_trees):
        # the items under every node of the tree, children before parents
        under, order, stack = {}, [], [int(roots[t])]
        while stack:
            v = stack.pop()
            reached[v] += 1
            order.append(v)
            if nodes[v, 0] == ref.SPLIT:
                stack += [int(nodes[v, 1]), int(nodes[v, 2])]
        for v in reversed(order):
            kind, a, b, flags = nodes[v]
            if kind == ref.LEAF:
                assert 1 <= b <= leaf and flags == 0
                under[v] = items[a:a + b]
                continue
            left, right = under.pop(int(a)), under.pop(int(b))
            assert len(left) and len(right)  # no split has an empty side
            under[v] = np.concatenate([left, right])
            assert len(under[v]) > leaf
            if flags & ref.FALLBACK:
                assert not normals[sn[v]].any() and offsets[sn[v]] == 0
                continue
            nrm = ref.pad8(normals[sn[v]].astype(np.float32))[0]
            off = offsets[sn[v]] if metric == L2 else None
            ml, mr = ref.margins(rows[left], nrm, off), ref.margins(rows[right], nrm, off)
            assert np.all(ml <= 0) and np.all(mr >= 0)  # (a margin of exactly 0 may be on either side)
            assert max(len(left), len(right)) <= 0.99 * len(under[v])
        assert np.array_equal(np.sort(under[int(roots[t])]), np.arange(N))  # the leaves partition 0..n-1
    assert np.all(reached == 1)
    f.close()


def test_margin_restatement_follows_the_header():
    """The vectorised restatement of the margin (tests/_annoy_ref.margins, which the split test above holds the library's
    sides to) against a scalar evaluation that follows the header word by word, at every row width the kernels
    distinguish."""
    rng = np.random.default_rng(1)
    for d in (3, 64, 100, 200, 1024):
        a = ref.pad8(rng.standard_normal((5, d)).astype(np.float16).astype(np.float32))
        b = ref.pad8(rng.standard_normal((5, d)).astype(np.float16).astype(np.float32))
        got = ref.margins(a, b)
        for r in range(5):
            lanes = [np.float32(0)] * 64
            for p in range(a.shape[1] // 8):
                for e in range(8):
                    lanes[p % 64] = np.float32(lanes[p % 64] + np.float32(a[r, p * 8 + e] * b[r, p * 8 + e]))
            for o in (32, 16, 8, 4, 2, 1):
                lanes = [np.float32(lanes[i] + lanes[i ^ o]) for i in range(64)]
            assert lanes[0] == got[r] and np.isfinite(got[r])


def test_forest_is_deterministic():
    x = _rows(64)
    for metric in (L2, COSINE):
        a = an.AnnoyForest.build(metric, x, 7, 0, seed=9, threads=1)
        b = an.AnnoyForest.build(metric, x, 7, 0, seed=9, threads=16)
        c = an.AnnoyForest.build(metric, x, 7, 0, seed=9, threads=16)
        assert _same(a, b) and _same(b, c)
        big = an.AnnoyForest.build(metric, x, 80, 0, seed=9, threads=0)
        n_nodes, n_splits = a.info()["n_nodes"], a.info()["n_splits"]
        assert np.array_equal(big.nodes[:n_nodes], a.nodes) and np.array_equal(big.items[:7 * N], a.items)
        assert np.array_equal(big.roots[:7], a.roots)
        assert np.array_equal(big.normals[:n_splits].view(np.uint16), a.normals.view(np.uint16))
        assert np.array_equal(big.offsets[:n_splits].view(np.uint32), a.offsets.view(np.uint32))
        other = an.AnnoyForest.build(metric, x, 7, 0, seed=10)
        assert not _same(a, other)


def test_identical_rows_terminate_through_fallback_splits():
    x = np.tile(_rows(16, n=1), (50, 1))
    for metric in (L2, COSINE):
        f = an.AnnoyForest.build(metric, x, 3, 2, seed=1)
        nodes = f.nodes
        splits = nodes[nodes[:, 0] == ref.SPLIT]
        assert len(splits) and np.all(splits[:, 3] == ref.FALLBACK) and not f.normals.any()
        leaves = nodes[nodes[:, 0] == ref.LEAF]
        assert leaves[:, 2].max() <= 2 and leaves[:, 2].sum() == 3 * 50


def _load_args(metric=L2, d=4, n=4, leaf=2):
    """Two trees over 4 items: a split with two leaves of 2; a chain."""
    nodes = np.array([[0, 1, 2, 0], [1, 0, 2, 0], [1, 2, 2, 0],
                      [0, 4, 5, 0], [1, 4, 1, 0], [0, 6, 7, 0], [1, 5, 1, 0], [1, 6, 2, 0]], np.int32)
    normals = np.zeros((3, d), np.float16)
    normals[:, 0] = 1
    return dict(metric=metric, d=d, n=n, leaf_size=leaf, nodes=nodes, normals=normals, offsets=np.zeros(3, np.float32),
                roots=np.array([0, 3], np.int32), items=np.array([0, 1, 2, 3, 3, 2, 1, 0], np.int32))


def test_load_accepts_a_forest_and_refuses_hostile_ones():
    good = _load_args()
    f = an.AnnoyForest.load(**good)
    assert np.array_equal(f.nodes, good["nodes"]) and np.array_equal(f.items, good["items"]) and f.info()["n_splits"] == 3

    def refused(match, code=EINVAL, **change):
        a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        for key, (idx, val) in change.items():
            a[key][idx] = val
        with pytest.raises(an.AnnoyError, match=match) as e:
            an.AnnoyForest.load(**a)
        assert f"error {code}:" in str(e.value)

    refused("child is out of range", nodes=((0, 1), 8))
    refused("child is out of range", nodes=((0, 2), -1))
    refused("reached twice", nodes=((5, 1), 3))        # a cycle: the chain's inner split points back at its root
    refused("reached twice", nodes=((0, 2), 1))        # a shared child
    refused("reached twice", nodes=((3, 1), 1))        # a child shared between two trees
    refused("reached twice", roots=(1, 0))             # the same root twice
    refused("twice in tree", items=(4, 2))             # an item twice (and one missing)
    refused("holds 3 of 4", nodes=((7, 2), 1))         # an item missing
    refused("outside 1..2", nodes=((1, 2), 3))         # an oversized leaf
    refused("outside 1..2", nodes=((1, 2), 0))
    refused("outside 0..n-1", items=(0, 4))
    refused("item range", nodes=((7, 1), 7))
    refused("unknown kind", nodes=((1, 0), 2))
    refused("flag", nodes=((0, 3), 2))
    refused("root is out of range", roots=(0, 8))
    refused("not finite", offsets=(0, np.inf))
    refused("not finite", normals=((0, 0), np.inf))
    lib = an._lib()
    a = good
    h = C.c_void_p()

    def raw(n=4, n_nodes=8, n_splits=3, n_items=8, metric=L2, d=4, n_trees=2, leaf=2):
        return lib.annoy_forest_load(metric, d, n, n_trees, leaf, n_nodes, a["nodes"].ctypes.data, n_splits,
                                     a["normals"].view(np.uint16).ctypes.data, a["offsets"].ctypes.data, a["roots"].ctypes.data, n_items,
                                     a["items"].ctypes.data, C.byref(h))

    assert raw() == 0 and h.value
    lib.annoy_forest_destroy(h)
    h = C.c_void_p()
    for kw in (dict(n=-4), dict(n_nodes=-1), dict(n_splits=-1), dict(n_items=-8), dict(n=0), dict(n_items=7), dict(n_splits=2),
               dict(metric=IP), dict(metric=7), dict(d=0), dict(d=1025), dict(n_trees=0), dict(n_trees=1025), dict(leaf=1),
               dict(leaf=2049), dict(n_nodes=1)):
        assert raw(**kw) == EINVAL and not h.value, kw
    assert raw(n=1 << 31) == ELIMIT and "2^31" in lib.annoy_last_error().decode()  # refused before any array is read
    assert raw(n=1 << 30, n_items=1 << 31) == ELIMIT
    assert raw(metric=IP) == EINVAL and "InnerProduct" in lib.annoy_last_error().decode()
    assert lib.annoy_forest_load(L2, 4, 4, 2, 2, 8, None, 3, None, None, None, 8, None, C.byref(h)) == EINVAL


def test_limits_are_refused_before_any_device_call():
    lib = an._lib()
    x = _rows(8, n=10)
    h = C.c_void_p()

    def build(metric=L2, d=8, n=10, n_trees=2, leaf=0, threads=1):
        return lib.annoy_forest_build(metric, d, n, x.ctypes.data, n_trees, leaf, 1, threads, C.byref(h))

    for kw in (dict(metric=IP), dict(metric=-1), dict(d=0), dict(d=1025), dict(n=0), dict(n=-1), dict(n_trees=0), dict(n_trees=1025),
               dict(leaf=1), dict(leaf=2049), dict(leaf=-1), dict(threads=-1), dict(threads=17)):
        assert build(**kw) == EINVAL and not h.value, kw
    assert build(n=1 << 31) == ELIMIT
    assert build(metric=IP) == EINVAL and "InnerProduct" in lib.annoy_last_error().decode()
    # the index: metric, shape and nulls before the device is touched (no device exists here)
    assert lib.annoy_index_build(0, IP, 8, 10, x.ctypes.data, None, 2, 0, 1, 1, C.byref(h)) == EINVAL
    assert "InnerProduct" in lib.annoy_last_error().decode()
    assert lib.annoy_index_build(0, L2, 2000, 10, x.ctypes.data, None, 2, 0, 1, 1, C.byref(h)) == EINVAL
    assert lib.annoy_index_build(-1, L2, 8, 10, x.ctypes.data, None, 2, 0, 1, 1, C.byref(h)) == EINVAL
    assert lib.annoy_index_from_forest(0, None, x.ctypes.data, None, C.byref(h)) == EINVAL
    out = np.zeros(4096, np.int64)
    o = out.ctypes.data
    addr = 0x1000  # never dereferenced: the numbers are refused first
    assert lib.annoy_search(addr, 1, x.ctypes.data, 1025, -1, o, o, o) == ELIMIT and "1024" in lib.annoy_last_error().decode()
    assert lib.annoy_search(addr, 1, x.ctypes.data, 0, -1, o, o, o) == EINVAL
    assert lib.annoy_search(addr, 0, x.ctypes.data, 1, -1, o, o, o) == EINVAL
    assert lib.annoy_search(addr, 1, x.ctypes.data, 1, -2, o, o, o) == EINVAL
    assert lib.annoy_search(None, 1, x.ctypes.data, 1, -1, o, o, o) == EINVAL and "null" in lib.annoy_last_error().decode()
    for fn, args in (("annoy_index_info", (None,) * 7), ("annoy_index_get_rows", (None, 0, 0, None)), ("annoy_index_forest", (None, None)),
                     ("annoy_last_candidates", (None,) * 5), ("annoy_last_stats", (None,) * 8), ("annoy_debug_set_limits", (None, 0, 0)),
                     ("annoy_forest_info", (None,) * 9), ("annoy_forest_get_nodes", (None, None))):
        assert getattr(lib, fn)(*args) == EINVAL, fn
    assert lib.annoy_index_destroy(None) == 0 and lib.annoy_forest_destroy(None) == 0
    with pytest.raises(ValueError, match="Not supported"):
        an.RawAnnoyIndexBuilder(8, 2, pkg.dense_ann.DistanceMetric.InnerProduct)
    with pytest.raises(ValueError, match="Not supported"):
        an.AnnoyQueryable.build(IP, x, 2)


def test_neighbours_to_request_follows_the_scala():
    """RawAnnoyQueryIndex.scala:124-138, by hand: Some(n) -> n / numOfTrees (Int division) unless that is below
    numOfNeighbours; None -> numOfNeighbours.  search_k is numOfTrees times that."""
    P = an.AnnoyRuntimeParams
    assert an.neighbours_to_request(10, P(None), 80) == 10
    assert an.neighbours_to_request(10, P(0), 80) == 10
    assert an.neighbours_to_request(10, P(799), 80) == 10      # 799 / 80 = 9 < 10
    assert an.neighbours_to_request(10, P(800), 80) == 10
    assert an.neighbours_to_request(10, P(879), 80) == 10      # 879 / 80 = 10
    assert an.neighbours_to_request(10, P(880), 80) == 11
    assert an.neighbours_to_request(10, P(50000), 80) == 625
    assert an.neighbours_to_request(1, P(20000), 7) == 2857
    assert an.neighbours_to_request(10, None, 3) == 10
    for k, nte, t in ((10, None, 80), (10, 0, 80), (10, 879, 80), (10, 880, 80), (1, 20000, 7), (200, 100, 7)):
        assert ref.search_k(t, k, nte) == t * an.neighbours_to_request(k, P(nte), t)


def test_builders_count_and_end():
    b = an.RawAnnoyIndexBuilder(4, 2, pkg.dense_ann.DistanceMetric.L2)
    assert [b.append(np.ones(4) * i) for i in range(3)] == [1, 2, 3]
    with pytest.raises(ValueError):
        b.append(np.ones(5))
    t = an.TypedAnnoyIndex.indexBuilder(4, 2, pkg.dense_ann.DistanceMetric.Cosine)
    assert t.append(77, np.ones(4)) == 1 and t.append(-5, np.ones(4)) == 2 and t._ids().tolist() == [77, -5]


def test_restatement_on_a_forest_followed_by_hand():
    """The two-tree forest of _load_args, d = 4, normals e0, Cosine (margin = q0).  Query q0 = 0.5: the queue starts
    (inf, 3), (inf, 0).  Pop 3 (node number decides): pushes (0.5, 5) and (-0.5, 4).  Pop 0: pushes (0.5, 2), (-0.5, 1).
    Pop 5 (0.5 ties, node 5 > 2): pushes (0.5, 7), (-0.5, 6).  Pop 7: leaf, items 1, 0.  Pop 2: leaf, items 2, 3: four
    collected.  With a budget of 3 the walk stops after node 2 (2 < 3 after node 7); with 2 it stops after node 7."""
    fa = _load_args(metric=COSINE)
    q = np.array([0.5, 0, 0, 0], np.float32)
    c, pops, coll = ref.walk(fa, q, 3)
    assert c.tolist() == [0, 1, 2, 3] and pops == 5 and coll == 4
    c, pops, coll = ref.walk(fa, q, 2)
    assert c.tolist() == [0, 1] and pops == 4 and coll == 2
    # q0 = 0: every bound below the roots is 0 (-0 counts as +0): strictly by node number, 7 6 5->, 4, then 2, 1
    c, pops, coll = ref.walk(fa, np.zeros(4, np.float32), 3)
    assert pops == 5 and coll == 3 and c.tolist() == [0, 1, 2]  # 3, 0, 5, 7 (items 1, 0), 6 (item 2)
    # q0 = -1: left sides first: 3, 0, then (1, 4) at bound 1: 4 (item 3), then 1 (items 0, 1)
    c, pops, coll = ref.walk(fa, np.array([-1, 0, 0, 0], np.float32), 3)
    assert pops == 4 and coll == 3 and c.tolist() == [0, 1, 3]


def test_numpy_builder_makes_loadable_forests():
    x = _rows(16, n=200)
    for metric in (L2, COSINE):
        fa = ref.numpy_forest(metric, ref.prepare(metric, x), 3, 0, seed=2)
        f = an.AnnoyForest.load(**fa)
        assert f.info()["n_nodes"] == len(fa["nodes"])
        q = ref.prepare(metric, x[:5])
        cands, _, _ = ref.walk_all(fa, q, 3 * 200)  # a budget that reaches every leaf
        assert all(np.array_equal(c, np.arange(200)) for c in cands)
        cands, pops, _ = ref.walk_all(fa, q, 1)     # a stored row descends to its own leaf
        assert all(i in cands[i] for i in range(5))


def test_forest_host_code_under_sanitizers(tmp_path):
    exe = str(tmp_path / "annoy_forest_host_check")
    # (the runtimes linked statically: the program then starts whatever else the process environment loads first)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-Wall", "-Wextra", "-ffp-contract=off", os.path.join(ROOT, "tests", "annoy_forest_host_check.cpp"),
                    os.path.join(ROOT, "the-algorithm_amd", "csrc", "annoy_forest.cpp"), "-o", exe, "-lpthread"], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-4000:]
    assert run.stdout.strip().endswith("ok: 144 forests, 0 failures"), run.stdout[-4000:]
