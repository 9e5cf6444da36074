"""The EditDistance index (include/edit_ann.h) on the device, against the numpy restatement of the plain dynamic programme
(tests/_edit_ref.py).  Every comparison is exact: int32 distances, int64 ids and counts."""
import importlib

import numpy as np
import pytest

import _edit_ref as ref

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


@pytest.fixture(scope="module")
def ed(pkg):
    return importlib.import_module(pkg.__name__ + ".edit_distance")


def expected(dist, ids, k):
    """(dist int32 [nq, k], ids int64 [nq, k], counts) of np.lexsort((position, ids, dist))[:k] per query, -1 past the count."""
    nq, n = dist.shape
    d, i = np.full((nq, k), -1, np.int32), np.full((nq, k), -1, np.int64)
    for q in range(nq):
        dd, ii = ref.top_k(dist[q], ids, k)
        d[q, :len(dd)], i[q, :len(ii)] = dd, ii
    return d, i, np.full(nq, min(k, n), np.int32)


def assert_search(index, queries, k, dist, ids):
    got = index.search(queries, k)
    want = expected(dist, ids, k)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int64 and got[2].dtype == np.int32
    for g, w, what in zip(got, want, ("distances", "ids", "counts")):
        assert np.array_equal(g, w), what
    return got


# ---- 6: the distance kernel at exact lengths ------------------------------------------------------------------------------
def test_pair_distances_on_the_length_grid_both_orientations(ed):
    rng = np.random.default_rng(61)
    lengths = tuple(sorted(ref.BOUNDARY_LENGTHS + (191, 192, 193)))
    a, b = ref.grid_pairs(rng, lengths, [np.array([1, 2], np.float32), np.arange(30, dtype=np.float32) + 1])
    assert len(a) == 2 * 2 * 17 * 17
    want = ref.pair_distances(a, b)
    assert len(np.unique(want)) > 20 and (want[1::2] <= 5 + 256).all()
    # a is the pattern (the word count follows len(a)), b the text: both orientations, so every word count meets every text length
    assert np.array_equal(ed.pair_distances(*ref.csr(a), *ref.csr(b), device=0), want)
    assert np.array_equal(ed.pair_distances(*ref.csr(b), *ref.csr(a), device=0), want)


def test_pair_distances_on_the_float_known_answers(ed):
    kats = ref.kats()
    a, b, want = [k[0] for k in kats], [k[1] for k in kats], np.array([k[2] for k in kats], np.int32)
    assert np.array_equal(ed.pair_distances(*ref.csr(a), *ref.csr(b), device=0), want)
    assert np.array_equal(ed.pair_distances(*ref.csr(b), *ref.csr(a), device=0), want)
    rng = np.random.default_rng(62)
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1.0], np.float32)
    x = ref.random_strings(rng, rng.integers(0, 200, 300), special)
    y = [ref.mutated(rng, s, int(n), special) for s, n in zip(x, rng.integers(0, 200, 300))]
    want = ref.pair_distances(x, y)
    assert np.array_equal(ed.pair_distances(*ref.csr(x), *ref.csr(y), device=0), want)
    assert np.array_equal(ed.Edit.distances(zip(y, x), device=0), want)


# ---- 7: the search against the full distance matrix ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def tied(ed):
    """4097 rows and 257 queries of length 0..40 over 4 symbols (empty rows and an empty query among them), unordered ids,
    and the restatement's distance matrix: every smaller case is a prefix of it."""
    rng = np.random.default_rng(7)
    alphabet = np.array([1, 2, 3, 4], np.float32)
    row_len, q_len = rng.integers(0, 41, 4097), rng.integers(0, 41, 257)
    row_len[[0, 5, 64, 1000, 4096]] = 0
    q_len[[0, 40]] = [0, 40]
    rows, queries = ref.random_strings(rng, row_len, alphabet), ref.random_strings(rng, q_len, alphabet)
    ids = rng.permutation(3 * 4097)[:4097].astype(np.int64) - 4097
    return rows, queries, ids, ref.distance_matrix(queries, rows)


@pytest.mark.parametrize("nq", [1, 33, 257])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 4097])
def test_search_equals_lexsort_of_the_restatement(ed, tied, n, nq):
    rows, queries, ids, dist = tied
    index = ed.EditBruteForceIndex(rows[:n], ids[:n])
    try:
        for k in (1, 10, 1024):
            got = assert_search(index, queries[:nq], k, dist[:nq, :n], ids[:n])
            if n >= 1000 and k == 10:
                assert (got[0][:, -1] == got[0][:, 0]).any(), "ties reach across the whole answer"
    finally:
        index.close()


def test_search_long_strings(ed):
    rng = np.random.default_rng(71)
    alphabet = np.arange(6, dtype=np.float32)
    rows = ref.random_strings(rng, rng.integers(200, 257, 130), alphabet)
    rows[7], rows[129] = rows[7][:256].copy(), np.resize(rows[129], 256)
    queries = [ref.mutated(rng, rows[i], n, alphabet) for i, n in ((3, 200), (7, 256), (50, 231), (129, 256))] + [rows[99].copy()]
    dist = ref.distance_matrix(queries, rows)
    assert dist[4, 99] == 0 and dist.max() > 100
    index = ed.EditBruteForceIndex(rows)
    try:
        for k in (1, 10, 130, 1024):
            assert_search(index, queries, k, dist, np.arange(130, dtype=np.int64))
    finally:
        index.close()


# ---- 8: tie masses ---------------------------------------------------------------------------------------------------------
def test_one_tie_mass_of_20000_rows(ed):
    rng = np.random.default_rng(8)
    row = np.array([3, 1, 4, 1, 5, 9, 2, 6], np.float32)
    query = np.array([3, 1, 4, 1, 5, 9, 2, 7, 7], np.float32)
    d = int(ref.pair_distances([query], [row])[0])
    assert d == 2
    ids = rng.permutation(20000).astype(np.int64) * 3 - 20000
    index = ed.EditBruteForceIndex([row] * 20000, ids)
    try:
        dist, got, counts = index.search([query], 1024)  # (a refusal would raise EditError)
        assert np.array_equal(got[0], np.sort(ids)[:1024]) and (dist == d).all() and counts.tolist() == [1024]
    finally:
        index.close()


@pytest.mark.parametrize("near", [15000, 500])
def test_two_tie_masses(ed, near):
    """`near` rows at distance 1 and 15,000 at distance 2, interleaved, ids shuffled.  With 15,000 near rows k = 1024 stays
    inside the first mass (k cannot exceed 1024, so it cannot reach past 15,000 rows); with 500 it takes the whole first mass
    and the 524 smallest ids of the second."""
    rng = np.random.default_rng(80 + near)
    query = np.array([1, 2, 3, 4, 5], np.float32)
    one, two = np.array([1, 2, 3, 4, 6], np.float32), np.array([1, 2, 3, 7, 6], np.float32)
    assert ref.pair_distances([query, query], [one, two]).tolist() == [1, 2]
    which = rng.permutation(np.r_[np.ones(near, np.int64), np.full(15000, 2, np.int64)])
    n = len(which)
    ids = rng.permutation(n).astype(np.int64)
    index = ed.EditBruteForceIndex([one if w == 1 else two for w in which], ids)
    try:
        for k in (1, 1024):
            dist, got, counts = index.search([query, two], k)
            want = expected(np.stack([which, 2 - which]).astype(np.int32), ids, k)
            assert np.array_equal(dist, want[0]) and np.array_equal(got, want[1]) and np.array_equal(counts, want[2])
        if near < 1024:
            assert (dist[0] == 1).sum() == near and (dist[0] == 2).sum() == 1024 - near
    finally:
        index.close()


# ---- 9: ids ----------------------------------------------------------------------------------------------------------------
def test_ids_unordered_negative_extreme_and_duplicated(ed):
    rng = np.random.default_rng(9)
    alphabet = np.array([1, 2, 3], np.float32)
    rows = ref.random_strings(rng, rng.integers(0, 12, 500), alphabet)
    queries = ref.random_strings(rng, rng.integers(0, 12, 20), alphabet)
    pool = np.array([I64_MIN, I64_MIN + 1, -5, -1, 0, 1, 7, 7, 2 ** 31, 2 ** 40, I64_MAX - 1, I64_MAX], np.int64)
    ids = pool[rng.integers(0, len(pool), 500)]
    ids[:2] = [I64_MAX, I64_MIN]
    dist = ref.distance_matrix(queries, rows)
    index = ed.EditBruteForceIndex(rows, ids)
    try:
        for k in (1, 7, 500, 1024):
            assert_search(index, queries, k, dist, ids)
    finally:
        index.close()
    # one id throughout: the order among equal ids is by position, which only the distances can show
    same = np.full(500, -3, np.int64)
    index = ed.EditBruteForceIndex(rows, same)
    try:
        assert_search(index, queries, 40, dist, same)
    finally:
        index.close()


# ---- 10: append ------------------------------------------------------------------------------------------------------------
def test_append_equals_build(ed):
    rng = np.random.default_rng(10)
    alphabet = np.array([1, 2, 3, 4], np.float32)
    x0 = ref.random_strings(rng, rng.integers(0, 41, 100), alphabet)
    x1 = ref.random_strings(rng, [60], alphabet)                       # longer than any stored row, into the partly filled tile
    x2 = ref.random_strings(rng, rng.integers(0, 41, 200), alphabet)
    i0 = rng.permutation(100).astype(np.int64) + 1000
    i1 = np.array([5000], np.int64)
    i2 = rng.permutation(2000)[:200].astype(np.int64)                  # below the stored maximum, some between the stored ids
    queries = ref.random_strings(rng, rng.integers(0, 41, 33), alphabet) + [x1[0].copy()]
    rows, ids = x0 + x1 + x2, np.r_[i0, i1, i2]
    dist = ref.distance_matrix(queries, rows)
    grown = ed.EditBruteForceIndex(x0, i0)
    whole = ed.EditBruteForceIndex(rows, ids)
    try:
        assert_search(grown, queries, 10, dist[:, :100], i0)           # (the search lays the rows on the device)
        grown.append(x1, i1)
        assert_search(grown, queries, 10, dist[:, :101], ids[:101])
        assert_search(grown, queries, 1024, dist[:, :101], ids[:101])
        grown.append(x2, i2)
        for k in (1, 10, 301, 1024):
            a, b = grown.search(queries, k), whole.search(queries, k)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
            assert_search(grown, queries, k, dist, ids)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(grown.rows(), whole.rows()))
        assert grown.info() == whole.info()
        # a refused append leaves the answers as they are
        before = grown.search(queries, 10)
        with pytest.raises(ed.EditError) as e:
            grown.append([np.zeros(257, np.float32)], [1])
        assert e.value.code == ed.EDIT_ELIMIT
        with pytest.raises(ed.EditError) as e:
            grown.append(x1)
        assert e.value.code == ed.EDIT_EINVAL
        assert all(x.tobytes() == y.tobytes() for x, y in zip(before, grown.search(queries, 10)))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(grown.rows(), whole.rows()))
    finally:
        grown.close()
        whole.close()
    # appends onto an empty index, with and without ids, in order and out of order
    for given in (ids, None):
        empty = ed.EditBruteForceIndex([], None if given is None else np.zeros(0, np.int64))
        try:
            assert empty.search(queries, 3)[2].tolist() == [0] * 34
            empty.append(x2, None if given is None else i2)
            empty.append(x0 + x1, None if given is None else np.r_[i0, i1])
            order = np.r_[101:301, 0:101]
            assert_search(empty, queries, 25, dist[:, order], ids[order] if given is not None else np.arange(301, dtype=np.int64))
        finally:
            empty.close()


# ---- 11: slices ------------------------------------------------------------------------------------------------------------
def test_query_slices_give_identical_bytes(ed):
    rng = np.random.default_rng(11)
    alphabet = np.array([1, 2, 3, 4], np.float32)
    rows = ref.random_strings(rng, rng.integers(0, 30, 130), alphabet)
    queries = ref.random_strings(rng, rng.integers(0, 30, 4097), alphabet)
    ids = rng.permutation(130).astype(np.int64)
    index = ed.EditBruteForceIndex(rows, ids)
    try:
        answers = []
        for per_pass in (1, 7, 1000, 0, 0):
            index.set_query_slice(per_pass)
            answers.append(index.search(queries, 10))
        for other in answers[1:]:
            assert all(x.tobytes() == y.tobytes() for x, y in zip(answers[0], other))
        some = np.r_[0:40, 4090:4097]
        dist = ref.distance_matrix([queries[q] for q in some], rows)
        want = expected(dist, ids, 10)
        assert np.array_equal(answers[0][0][some], want[0]) and np.array_equal(answers[0][1][some], want[1])
    finally:
        index.close()


# ---- 12: the empty index, the counters -------------------------------------------------------------------------------------
def test_empty_index_and_last_stats(ed):
    rng = np.random.default_rng(12)
    alphabet = np.array([1, 2], np.float32)
    queries = ref.random_strings(rng, rng.integers(0, 50, 19), alphabet)
    empty = ed.EditBruteForceIndex([])
    try:
        dist, ids, counts = empty.search(queries, 5)
        assert counts.tolist() == [0] * 19 and (dist == -1).all() and (ids == -1).all()
        assert empty.last_stats() == {"pairs": 0, "cell_updates": 0}
        assert empty.query("abc", 3) == [] and empty.query_with_distance("abc", 3) == []
    finally:
        empty.close()
    rows = ref.random_strings(rng, rng.integers(0, 50, 77), alphabet)
    index = ed.EditBruteForceIndex(rows)
    try:
        index.search(queries, 5)
        cells = sum(len(q) * len(r) for q in queries for r in rows)
        assert index.last_stats() == {"pairs": 19 * 77, "cell_updates": cells}
        t = index.last_timing()
        assert t["distance_ms"] > 0 and t["select_ms"] > 0
        # the Queryable shape, on strings
        words = ed.EditBruteForceIndex(["kitten", "sitting", "mitten", "", "bitten"], ids=[50, 40, 30, 20, 10])
        try:
            got = words.query_with_distance("kitten", 4)
            assert got == [(50, 0), (10, 1), (30, 1), (40, 3)] and all(isinstance(d, ed.EditDistance) for _, d in got)
            assert words.query("", 2) == [20, 10]
        finally:
            words.close()
    finally:
        index.close()
