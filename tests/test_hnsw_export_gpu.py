"""The graph export (hnsw_index_graph_size / hnsw_index_graph): which HnswNode(level, item) keys it shows, that it shows them again
after an append, and that calling it changes nothing a later append, update or search can see.

d = 8, max_m = 2 (lists of 4 at level 0, 2 above), L2, every level given: the smallest shapes that have empty keys, rows
without keys, several layers and more than one round."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, MAX_M = 8, 2


def _entries(g):
    lv, it, off, nb = g[:4]
    return {(int(lv[e]), int(it[e])): nb[off[e]:off[e + 1]].tolist() for e in range(len(lv))}


def _same_graph(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4] and a[5] == b[5]


def test_a_loaded_graph_comes_back_entry_for_entry_and_its_keys_outlive_an_append(pkg):
    m = pkg.dense_ann.DistanceMetric.L2
    x = np.random.default_rng(1).standard_normal((10, D)).astype(np.float32)
    # (level, item): list.  (0, 3) and (1, 5) are keys with empty lists that no list names; row 4 has no key at all; item 0,
    # the entry point, has no key on level 2, where (2, 2) names it
    given = [((0, 0), [1, 2]), ((0, 1), [0]), ((0, 2), [0, 1]), ((0, 3), []), ((0, 5), [0]),
             ((1, 0), [2]), ((1, 2), [0]), ((1, 5), []),
             ((2, 2), [0])]
    lv = np.array([k[0] for k, _ in given], np.int32)
    it = np.array([k[1] for k, _ in given], np.int64)
    off = np.concatenate([[0], np.cumsum([len(l) for _, l in given])]).astype(np.int64)
    nb = np.array([v for _, l in given for v in l], np.int64)
    ix = pkg.hnsw_ann.Hnsw.from_graph(m, x[:6], (lv, it, off, nb, 0, 2), max_m=MAX_M)
    try:
        g = ix.graph()
        assert g[4] == 0 and g[5] == 2
        assert np.array_equal(g[0], lv) and np.array_equal(g[1], it), "the same keys in the same order"
        assert np.array_equal(g[2], off) and np.array_equal(g[3], nb), "the same lists"
        ix.append(x[6:], levels=np.array([0, 1, 0, 3], np.int32))
        after = _entries(ix.graph())
        assert set(after) >= {k for k, _ in given}, "every old key is still exported"
        assert after[(0, 3)] == [] and after[(1, 5)] == [], "an empty key nobody linked to is still an empty entry"
        g = ix.graph()
        assert g[4] == 9 and g[5] == 3, "the row above maxLevel is the entry point"
    finally:
        ix.close()


def test_exports_are_not_observable(pkg):
    m = pkg.dense_ann.DistanceMetric.L2
    rng = np.random.default_rng(2)
    x = rng.standard_normal((96, D)).astype(np.float32)
    levels = np.minimum(60, (-np.log(1.0 - rng.random(96)) / np.log(MAX_M)).astype(np.int32)).astype(np.int32)
    assert levels[:64].max() >= 2, "at least three layers"
    first = int(np.argmax(levels[:64]))  # the build's entry point, which holds no key of its own, is among the updated rows
    keys = np.concatenate([[first], rng.choice(np.delete(np.arange(96), first), 15, replace=False)]).astype(np.int64)
    rows = rng.standard_normal((16, D)).astype(np.float32)
    queries = rng.standard_normal((8, D)).astype(np.float32)
    out = []
    for export_after_every_step in (True, False):
        ix = pkg.hnsw_ann.Hnsw.build(m, x[:64], max_m=MAX_M, ef_construction=32, levels=levels[:64], gpu=True, batch=8)
        try:
            if export_after_every_step:
                ix.graph()
            ix.append(x[64:], ef_construction=32, levels=levels[64:], batch=8)
            if export_after_every_step:
                ix.graph()
            assert ix.update(rows, keys, ef_construction=32, batch=8) == 0
            out.append((ix.graph(), ix.update_stats(), ix.search(queries, 5, 32)))
        finally:
            ix.close()
    (ga, sa, ra), (gb, sb, rb) = out
    assert _same_graph(ga, gb), "the final graphs"
    assert sa == sb and sa["rounds"] == 2, "update_stats()"
    assert all(np.array_equal(p, q) for p, q in zip(ra, rb)), "the search answers"


def test_an_empty_index_exports_nothing_and_then_the_schedule_of_its_first_append(pkg):
    m = pkg.dense_ann.DistanceMetric.L2
    x = np.random.default_rng(3).standard_normal((3, D)).astype(np.float32)
    ix = pkg.hnsw_ann.Hnsw.build(m, x[:0], max_m=MAX_M, levels=np.zeros(0, np.int32), gpu=True)
    try:
        g = ix.graph()
        assert len(g[0]) == 0 and len(g[3]) == 0 and g[2].tolist() == [0] and g[4] == -1
        # row 1 is first in order: the entry point, never wired, so it has no key on level 1 and one on level 0 only through the
        # back links of rows 0 and 2 (rounds of one row each); every list has room, so nothing is re-selected
        ix.append(x, levels=np.array([0, 1, 0], np.int32))
        g = ix.graph()
        assert g[4] == 1 and g[5] == 1
        e = _entries(g)
        assert sorted(e) == [(0, 0), (0, 1), (0, 2)]
        assert {k: sorted(v) for k, v in e.items()} == {(0, 0): [1, 2], (0, 1): [0, 2], (0, 2): [0, 1]}
    finally:
        ix.close()
