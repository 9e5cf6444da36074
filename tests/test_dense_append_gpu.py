"""BruteForceIndex.append on the device (dann_index_append): a search on build(X0) + append(X1) + ... returns the ids, the
distance bits and the counts of a search on build(X0 ++ X1 ++ ...), in the fast and the exact mode, whatever order the ids
arrive in and however the appends cut the tiles."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CUTS = [700, 1000, 1024, 2524, 2525]  # inside a tile, to a tile edge (512-row tiles at d <= 256), across tiles, one row


def _data(seed, n=CUTS[-1], d=64):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[800] = x[5]  # equal rows: equal scores, ordered by id on both sides
    x[1500] = x[20]
    x[2524] = x[5]
    q = np.concatenate([rng.standard_normal((40, d)).astype(np.float32), x[[5, 20, 900, 2000]]])
    return rng, x, q


def _keys(kind, rng, n):
    if kind is None:
        return None
    if kind == "increasing":
        return np.arange(n, dtype=np.int64) * 3 + 11
    return rng.permutation(10 * n)[:n].astype(np.int64) - 5 * n  # any order, negative ones too


def _same(a, b):
    ids_a, dist_a, cnt_a = a
    ids_b, dist_b, cnt_b = b
    assert np.array_equal(cnt_a, cnt_b)
    for i in range(len(cnt_a)):
        assert np.array_equal(ids_a[i, :cnt_a[i]], ids_b[i, :cnt_b[i]]), i
        assert np.array_equal(dist_a[i, :cnt_a[i]].view(np.int32), dist_b[i, :cnt_b[i]].view(np.int32)), i


@pytest.mark.parametrize("metric", ["L2", "Cosine", "InnerProduct"])
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("keys", [None, "increasing", "shuffled"])
def test_search_after_appends_is_search_on_one_build(pkg, metric, exact, keys):
    B = pkg.dense_ann.BruteForceIndex
    m = getattr(pkg.dense_ann.DistanceMetric, metric)
    rng, x, q = _data(7)
    ids = _keys(keys, rng, len(x))
    sl = (lambda a, b: None) if ids is None else (lambda a, b: ids[a:b])
    one = B.build(m, x, ids, exact=exact)
    grown = B.build(m, x[:CUTS[0]], sl(0, CUTS[0]), exact=exact)
    try:
        for a, b in zip(CUTS[:-1], CUTS[1:]):
            grown.append(x[a:b], sl(a, b))
            assert grown.n == b
            part = B.build(m, x[:b], sl(0, b), exact=exact)
            try:
                _same(grown.search(q, 10), part.search(q, 10))
            finally:
                part.close()
        for k in (1, 10, 200):
            _same(grown.search(q, k), one.search(q, k))
        if keys != "shuffled":  # positions are the build's
            assert np.array_equal(grown.stored_vectors(), one.stored_vectors())
    finally:
        one.close(); grown.close()


def test_reserve_then_append_and_a_synthetic_index(pkg):
    B = pkg.dense_ann.BruteForceIndex
    m = pkg.dense_ann.DistanceMetric.L2
    rng, x, q = _data(3, d=48)
    one = B.build(m, x)
    grown = B.build(m, x[:10])
    try:
        grown.reserve(len(x))
        grown.reserve(5)  # never shrinks
        for a in range(10, len(x), 333):
            grown.append(x[a:a + 333])
        _same(grown.search(q, 50), one.search(q, 50))
    finally:
        one.close(); grown.close()
    syn = B.synthetic(m, 3000, 64, seed=4)
    try:
        base = syn.stored_vectors()
        more = rng.standard_normal((700, 64)).astype(np.float32)
        syn.append(more)
        assert syn.n == 3700
        ids, dist, cnt = syn.search(more[:20], 1)
        assert np.array_equal(ids[:, 0], 3000 + np.arange(20))
        assert np.array_equal(syn.stored_vectors(0, 3000), base)
    finally:
        syn.close()


def test_append_errors_leave_the_index_unchanged(pkg):
    B, DannError = pkg.dense_ann.BruteForceIndex, pkg.dense_ann.DannError
    m = pkg.dense_ann.DistanceMetric.Cosine
    rng, x, q = _data(9)
    keyed = B.build(m, x[:1000], np.arange(1000, dtype=np.int64))
    plain = B.build(m, x[:1000])
    try:
        before_k, before_p = keyed.search(q, 20), plain.search(q, 20)
        with pytest.raises(DannError, match="ids"):
            keyed.append(x[1000:1100])
        with pytest.raises(DannError, match="ids"):
            plain.append(x[1000:1100], np.arange(100, dtype=np.int64))
        with pytest.raises(ValueError):
            keyed.append(x[1000:1100, :32], np.arange(100, dtype=np.int64))
        with pytest.raises(ValueError):
            keyed.append(x[1000:1100], np.arange(99, dtype=np.int64))
        assert keyed.n == 1000 and plain.n == 1000
        _same(keyed.search(q, 20), before_k)
        _same(plain.search(q, 20), before_p)
    finally:
        keyed.close(); plain.close()
