"""The grouped index on the device (include/grouped_ann.h) against the float64 restatement tests/_grouped_ref.py.
Tolerance: the project's 1e-5 / 1e-5 on distances (tests/_ivf_ref.py); ids must agree wherever the restatement's distances
are further apart than that.  The invariance tests compare bytes."""
import numpy as np
import pytest

import _grouped_ref as ref

pytestmark = pytest.mark.gpu

RTOL, ATOL = ref.RTOL, ref.ATOL
METRICS = ["L2", "Cosine", "InnerProduct"]
CAP = 8192    # the survivor buffer of a query (grouped_ann.h: the tie limit)
CHUNK = 4096  # queries per search chunk (the dense search's, ivf_core.h search_chunks)
ELIMIT = 3

SIZES = [0, 1, 31, 32, 33, 64, 200, 1000, 4096, 9000]
D = 64


def _metric(pkg, name):
    return getattr(pkg.dense_ann.DistanceMetric, name)


def _close(got, want):
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


def _corpus(rng, sizes, d):
    """Rows of groups of the given sizes, shuffled so that groups interleave; ids a random permutation of distinct values."""
    groups = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    groups = groups[rng.permutation(len(groups))]
    n = len(groups)
    x = rng.standard_normal((n, d)).astype(np.float32)
    ids = rng.permutation(n).astype(np.int64) * 7 + 1_000_000_007
    return x, ids, groups


class _Case:
    def __init__(self):
        rng = np.random.default_rng(20)
        self.x, self.ids, self.groups = _corpus(rng, SIZES, D)
        ng = len(SIZES)
        # one query on every group, 33 and 65 on two of them (the tile boundary; the second on the group that exceeds the
        # survivor buffer), the two kinds of absent key, the rest random
        qg = list(range(ng)) + [6] * 33 + [9] * 65 + [-1, ng]
        qg += rng.integers(0, ng, 200 - len(qg)).tolist()
        self.qg = np.array(qg, np.int32)[rng.permutation(len(qg))]
        self.q = rng.standard_normal((len(qg), D)).astype(np.float32)
        self.order = np.argsort(self.ids)
        self.built = {}

    def index(self, pkg, metric):
        """(device index, restatement) of the metric, built once."""
        if metric not in self.built:
            m = _metric(pkg, metric)
            ix = _build(pkg, m, len(SIZES), self.x, self.ids, self.groups)
            self.built[metric] = (ix, ref.GroupedRef(int(m), len(SIZES), self.x, self.ids, self.groups))
        return self.built[metric]

    def row_of(self, ids):
        pos = np.searchsorted(self.ids[self.order], ids)
        assert np.array_equal(self.ids[self.order][pos], ids), "every returned id is an id of the index"
        return self.order[pos]


@pytest.fixture(scope="module")
def case():
    c = _Case()
    yield c
    for ix, _ in c.built.values():
        ix.close()


def _build(pkg, m, n_groups, x, ids, groups):
    """GroupedIndex over group numbers: the keys are the numbers' decimal strings, every group present in the table."""
    return pkg.grouped_ann.GroupedIndex.build_numbered(x, ids, groups, [str(i) for i in range(n_groups)], m)


def _check_answer(gref, rows_prepared, row_of, groups, q, qg, k, got):
    """Every returned position of every query against the restatement."""
    got_ids, got_dist, cnt = got
    sizes = gref.group_sizes()
    want = gref.search(q, qg, k)
    qp = ref.prepare(gref.metric, q)
    for i, (r_ids, r_dist, nxt) in enumerate(want):
        known = 0 <= qg[i] < gref.n_groups
        m = min(k, int(sizes[qg[i]])) if known else 0
        assert cnt[i] == m == len(r_ids), f"query {i}: count {cnt[i]}, group size says {m}"
        if m == 0:
            continue
        ids_i, dist_i = got_ids[i, :m], got_dist[i, :m]
        rows = row_of(ids_i)
        assert np.all(groups[rows] == qg[i]), f"query {i}: a row of another group"
        _close(dist_i, ref.distances(gref.metric, qp[i:i + 1], rows_prepared[rows])[0])
        _close(dist_i, r_dist)
        assert len(set(ids_i.tolist())) == m, "no id twice"
        clear = ref.clear_positions(r_dist, nxt)
        assert np.array_equal(ids_i[clear], r_ids[clear])


@pytest.mark.parametrize("k", [1, 10, 200, 1024])
@pytest.mark.parametrize("metric", METRICS)
def test_mixed_batch_against_restatement(pkg, case, metric, k):
    ix, gref = case.index(pkg, metric)
    assert np.array_equal(ix.group_sizes(), SIZES)
    assert ix.info() == {"n": sum(SIZES), "d": D, "metric": int(_metric(pkg, metric)), "n_groups": len(SIZES)}
    got = ix.search_groups(case.q, case.qg, k)
    _check_answer(gref, gref.rows, case.row_of, case.groups, case.q, case.qg, k, got)
    st = ix.last_stats()
    known = (case.qg >= 0) & (case.qg < len(SIZES))
    assert st["rows_scanned"] == int(np.asarray(SIZES)[case.qg[known]].sum())
    assert SIZES[-1] > CAP and SIZES[-1] > 2 * st["segment_rows"], "the largest group overflows the buffer and spans three segments"
    # per group with queries and rows: tiles = ceil(queries / 32), work items = tiles x ceil(rows / segment)
    per = np.bincount(case.qg[known], minlength=len(SIZES))
    tiles = -(-per // 32)
    segs = -(-np.asarray(SIZES) // st["segment_rows"])
    assert st["tiles"] == int(tiles.sum())
    assert st["work_items"] == int((tiles * segs).sum()) and st["work_items"] > st["tiles"]
    assert 1 <= st["rounds"] <= 17


@pytest.mark.parametrize("metric", METRICS)
def test_dimension_256(pkg, metric):
    m = _metric(pkg, metric)
    rng = np.random.default_rng(21)
    sizes = [3, 0, 70, 2500]
    x, ids, groups = _corpus(rng, sizes, 256)
    qg = np.array([0, 1, 2, 3, 4, -7] + rng.integers(0, 4, 34).tolist(), np.int32)
    q = rng.standard_normal((len(qg), 256)).astype(np.float32)
    ix = _build(pkg, m, len(sizes), x, ids, groups)
    gref = ref.GroupedRef(int(m), len(sizes), x, ids, groups)
    order = np.argsort(ids)

    def row_of(a):
        return order[np.searchsorted(ids[order], a)]

    for k in (10, 100):
        _check_answer(gref, gref.rows, row_of, groups, q, qg, k, ix.search_groups(q, qg, k))
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_ties_answer_in_id_order_with_equal_bits(pkg, metric):
    m = _metric(pkg, metric)
    rng = np.random.default_rng(22)
    row = rng.standard_normal(D).astype(np.float32)
    x = np.concatenate([np.tile(row, (40, 1)), rng.standard_normal((50, D)).astype(np.float32)])
    ids = np.concatenate([rng.permutation(40) * 3 + 5, 1000 + np.arange(50)]).astype(np.int64)
    groups = np.array([1] * 40 + [0] * 50, np.int32)
    ix = _build(pkg, m, 2, x, ids, groups)
    q = rng.standard_normal((3, D)).astype(np.float32)
    got_ids, got_dist, cnt = ix.search_groups(q, [1, 1, 1], 40)
    assert cnt.tolist() == [40, 40, 40]
    for i in range(3):
        assert got_ids[i].tolist() == sorted(ids[:40].tolist())
        assert len(set(got_dist[i].view(np.uint32).tolist())) == 1, "one row, one distance"
    ix.close()


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
            and np.array_equal(a[2], b[2]))


@pytest.mark.parametrize("metric", METRICS)
def test_a_query_alone_answers_as_in_the_batch(pkg, case, metric):
    ix, _ = case.index(pkg, metric)
    k = 10
    batch = ix.search_groups(case.q, case.qg, k)
    for i in range(len(case.qg)):
        alone = ix.search_groups(case.q[i:i + 1], case.qg[i:i + 1], k)
        assert _same(alone, tuple(a[i:i + 1] for a in batch)), f"query {i} (group {case.qg[i]})"


@pytest.mark.parametrize("metric", METRICS)
def test_other_groups_and_rebuilds_do_not_change_the_bytes(pkg, case, metric):
    m = _metric(pkg, metric)
    ix, _ = case.index(pkg, metric)
    k = 200
    batch = ix.search_groups(case.q, case.qg, k)
    # the 1000-row group alone, as group 0 of its own index
    sel = case.groups == 7
    own = _build(pkg, m, 1, case.x[sel], case.ids[sel], np.zeros(int(sel.sum()), np.int32))
    mine = np.flatnonzero(case.qg == 7)
    assert len(mine) >= 2
    got = own.search_groups(case.q[mine], np.zeros(len(mine), np.int32), k)
    assert _same(got, tuple(a[mine] for a in batch))
    own.close()
    # a second build from the same arguments
    again = _build(pkg, m, len(SIZES), case.x, case.ids, case.groups)
    assert _same(again.search_groups(case.q, case.qg, k), batch)
    again.close()


def test_null_ids_are_positions(pkg, case):
    m = _metric(pkg, "L2")
    n = 3000
    x, groups = case.x[:n], (case.groups[:n] % 3).astype(np.int32)
    ix = _build(pkg, m, 3, x, None, groups)
    gref = ref.GroupedRef(int(m), 3, x, None, groups)
    q, qg = case.q[:20], np.arange(20, dtype=np.int32) % 3
    _check_answer(gref, gref.rows, lambda a: a, groups, q, qg, 10, ix.search_groups(q, qg, 10))
    # a stored row as the query finds its own position
    got_ids, _, _ = ix.search_groups(x[17:18], groups[17:18], 1)
    assert got_ids[0, 0] == 17
    ix.close()


def test_tie_limit_is_reported_and_the_index_stays_usable(pkg):
    m = _metric(pkg, "InnerProduct")
    rng = np.random.default_rng(23)
    row = rng.standard_normal(D).astype(np.float32)
    other = rng.standard_normal((100, D)).astype(np.float32)
    x = np.concatenate([np.tile(row, (9000, 1)), other])
    groups = np.array([0] * 9000 + [1] * 100, np.int32)
    ix = _build(pkg, m, 2, x, None, groups)
    q = rng.standard_normal((2, D)).astype(np.float32)
    with pytest.raises(pkg.grouped_ann.GroupedError, match=str(CAP)) as e:
        ix.search_groups(q, [1, 0], 1)
    assert e.value.code == ELIMIT
    gref = ref.GroupedRef(int(m), 2, x, None, groups)
    qg = np.array([1, 1], np.int32)
    _check_answer(gref, gref.rows, lambda a: a, groups, q, qg, 5, ix.search_groups(q, qg, 5))
    ix.close()


def test_more_queries_than_a_chunk(pkg):
    m = _metric(pkg, "L2")
    rng = np.random.default_rng(24)
    sizes = [5, 40, 0, 17]
    x, ids, groups = _corpus(rng, sizes, 16)
    nq = CHUNK + 1
    q = rng.standard_normal((nq, 16)).astype(np.float32)
    qg = rng.integers(-1, 5, nq).astype(np.int32)
    ix = _build(pkg, m, len(sizes), x, ids, groups)
    whole = ix.search_groups(q, qg, 3)
    first = ix.search_groups(q[:CHUNK], qg[:CHUNK], 3)
    last = ix.search_groups(q[CHUNK:], qg[CHUNK:], 3)
    assert _same(tuple(a[:CHUNK] for a in whole), first) and _same(tuple(a[CHUNK:] for a in whole), last)
    gref = ref.GroupedRef(int(m), len(sizes), x, ids, groups)
    tail = slice(CHUNK - 40, nq)
    order = np.argsort(ids)
    _check_answer(gref, gref.rows, lambda a: order[np.searchsorted(ids[order], a)], groups, q[tail], qg[tail], 3,
                  tuple(a[tail] for a in whole))
    ix.close()


def test_grouped_queryable(pkg):
    ga = pkg.grouped_ann
    m = _metric(pkg, "Cosine")
    rng = np.random.default_rng(25)
    keys = ["en"] * 30 + ["fr"] * 5 + ["ja"] * 12
    perm = rng.permutation(len(keys))
    keys = [keys[i] for i in perm]
    x = rng.standard_normal((len(keys), 32)).astype(np.float32)
    ids = (rng.permutation(len(keys)) + 100).astype(np.int64)
    ix = ga.GroupedIndex.build(x, ids, keys, m)
    assert ix.keys == list(dict.fromkeys(keys))
    assert dict(zip(ix.keys, ix.group_sizes().tolist())) == {"en": 30, "fr": 5, "ja": 12}
    qa = ga.GroupedQueryable(ix)
    q = rng.standard_normal(32).astype(np.float32)
    table, groups = ga.key_table(keys)
    gref = ref.GroupedRef(int(m), len(table), x, ids, groups)
    for key in ("en", "fr", "ja"):
        got = qa.query_with_distance(q, 8, None, key)
        r_ids, r_dist, nxt = gref.search(q[None, :], [table.index(key)], 8)[0]
        assert len(got) == min(8, keys.count(key))
        assert all(keys[int(np.flatnonzero(ids == i)[0])] == key for i, _ in got)
        _close([dd for _, dd in got], r_dist)
        clear = ref.clear_positions(r_dist, nxt)
        assert np.array_equal(np.array([i for i, _ in got])[clear], r_ids[clear])
        assert qa.query(q, 8, object(), key) == [i for i, _ in got]
    assert qa.query_with_distance(q, 8, None, "de") == [] and qa.query(q, 8, None, "de") == []
    assert qa.query_with_distance(q, 8, None, None) == [] and qa.query(q, 8, None) == []
    batch = qa.batch_query_with_distance(np.stack([q, q, q, q]), 8, None, ["fr", None, "en", "xx"])
    assert batch[0] == qa.query_with_distance(q, 8, None, "fr") and batch[2] == qa.query_with_distance(q, 8, None, "en")
    assert batch[1] == [] and batch[3] == []
    assert qa.batch_query(np.stack([q, q]), 8, None, ["ja", "fr"]) == [qa.query(q, 8, None, "ja"), qa.query(q, 8, None, "fr")]
    ix.close()
