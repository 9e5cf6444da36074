"""IVF-SQ8 on the device (include/ivfsq_ann.h) against the restatement tests/_ivfsq_ref.py, fed with what the index exports
(codes, ranges, assignment, probes) -- never with the device's own answers.  Tolerance: the project's 1e-5 / 1e-5 on
distances; ids must agree wherever the restatement's distances are further apart than that.  PARITY UNPINNED against
Faiss (not vendored in the reference), as the header says."""
import importlib

import numpy as np
import pytest

import _ivfsq_ref as ref

pytestmark = pytest.mark.gpu

RTOL, ATOL = ref.RTOL, ref.ATOL
METRICS = ["L2", "Cosine", "InnerProduct"]


@pytest.fixture(scope="module")
def sq(pkg):
    return importlib.import_module(pkg.__name__ + ".scalar_quantizer")


def _metric(pkg, name):
    return getattr(pkg.dense_ann.DistanceMetric, name)


def _close(got, want):
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


def _restated(ix, metric, queries, k):
    """The restatement's answer over the index's exports: per query (ids, distances, the (k+1)-th distance)."""
    a_ids, cells = ix.assignment()
    vmin, vdiff = ix.ranges()
    dist = ref.distances(int(metric), ref.prepare(int(metric), queries), ix.codes(), vmin, vdiff)
    return ref.search_probed(dist, a_ids, cells, ix.last_probes(), k)


def _unclear_share(want):
    total = sum(len(r_ids) for r_ids, _, _ in want)
    return sum(int((~ref.clear_positions(r_dist, nxt)).sum()) for _, r_dist, nxt in want) / max(total, 1)


def _check_search(ix, metric, queries, k, nprobe, cap=None):
    """Counts and distances at every returned position, ids at the clear ones.  cap: the share of unclear positions, from
    the restatement alone, is bounded before any id is compared."""
    got_ids, got_dist, cnt = ix.search(queries, k, nprobe)
    want = _restated(ix, metric, queries, k)
    share = _unclear_share(want)
    print(f"k {k} nprobe {nprobe}: unclear share {share:.4f}")
    if cap is not None:
        assert share <= cap
    for q, (r_ids, r_dist, nxt) in enumerate(want):
        m = len(r_ids)
        assert cnt[q] == m, f"query {q}: count {cnt[q]} != {m}"
        _close(got_dist[q, :m], r_dist)
        assert (np.diff(got_dist[q, :m]) >= 0).all(), "ascending"
        assert not got_dist[q, m:].any() and not got_ids[q, m:].any(), "slots past the count are zeros"
        clear = ref.clear_positions(r_dist, nxt)
        assert np.array_equal(got_ids[q, :m][clear], r_ids[clear])
        assert len(set(got_ids[q, :m].tolist())) == m, "no id twice"
    return got_ids, got_dist, cnt


# ---- the known answer by hand -------------------------------------------------------------------------------------------
def test_known_answer_by_hand(pkg, sq):
    d, j = 16, 5
    ix = sq.FaissIvfSq8.load(_metric(pkg, "InnerProduct"), np.zeros((1, d), np.float32), np.zeros(d, np.float32),
                             np.full(d, 255, np.float32))
    x = np.zeros((4, d), np.float32)
    x[:, j] = [0.5, 3.7, 254.9, 300.0]  # fp16: 0.5, 3.69921875, 254.875, 300 -> codes 0, 3, 254, 255 (clipped)
    ix.add(x, [40, 30, 20, 10])
    codes = ix.codes()
    assert codes[:, j].tolist() == [0, 3, 254, 255] and not np.delete(codes, j, axis=1).any()
    assert np.array_equal(ix.codes(1, 2), codes[1:3])
    q = np.zeros((1, d), np.float32)
    q[0, j] = 1.0
    ids, dist, cnt = ix.search(q, 4, 1)
    # s = 1, b_q = 0.5: the scores are code + 0.5, exactly
    assert cnt.tolist() == [4] and ids[0].tolist() == [10, 20, 30, 40]
    assert dist[0].tolist() == [1 - 255.5, 1 - 254.5, 1 - 3.5, 1 - 0.5]
    vmin, vdiff = ix.ranges()
    assert not vmin.any() and (vdiff == 255).all()
    assert pkg.ivf_ann.FaissQueryable(ix, ix.metric).queryWithDistance(q[0], 2, pkg.ivf_ann.FaissParams(nprobe=1)) == \
        [(10, -254.5), (20, -253.5)]
    ix.close()


# ---- codes and ranges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [16, 48, 272])
def test_codes_and_ranges_equal_the_restatement(pkg, sq, metric, d):
    m = _metric(pkg, metric)
    rng = np.random.default_rng(100 + d)
    train = (rng.standard_normal((2000, d)) * rng.uniform(0.05, 4.0, d)).astype(np.float32)
    train[:, 3] = 0.0  # constant over the training set (Cosine: a zero stays a zero)
    train[::2, 3] = -0.0
    ix = sq.FaissIvfSq8.train(m, 8, train, niter=1, seed=5)
    vmin, vdiff = ix.ranges()
    w_vmin, w_vdiff = ref.ranges(ref.prepare(int(m), train))
    assert vmin.tobytes() == w_vmin.tobytes() and vdiff.tobytes() == w_vdiff.tobytes()
    assert vdiff[3] == 0 and (np.delete(vdiff, 3) > 0).all()
    # rows inside the range, and rows beyond it in both directions (one dominant component each: beyond it under Cosine too)
    x = (rng.standard_normal((700, d)) * rng.uniform(0.05, 4.0, d)).astype(np.float32)
    x[:, 3] = rng.standard_normal(700)
    for i in range(2 * d):
        x[i, i % d] = (50.0 if i < d else -50.0) * (1 + i % 7)
    ix.add(x[:300])
    ix.add(x[300:])
    want = ref.encode(ref.prepare(int(m), x), w_vmin, w_vdiff)
    got = ix.codes()
    assert got.dtype == np.uint8 and got.shape == (700, d)
    assert got.tobytes() == want.tobytes()
    assert not got[:, 3].any(), "a component with step 0 has code 0"
    assert (got[np.arange(d), np.arange(d)][np.arange(d) != 3] == 255).all() and not got[d + np.arange(d), np.arange(d)].any(), "clipping"
    ix.close()


# ---- the twin -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_twin_of_the_flat_index(pkg, sq, metric):
    m = _metric(pkg, metric)
    rng = np.random.default_rng(21)
    n, d, nlist = 5000, 64, 32
    x = rng.standard_normal((n, d)).astype(np.float32)
    ids = rng.permutation(n).astype(np.int64) * 5 + 3
    q = rng.standard_normal((64, d)).astype(np.float32)
    flat = pkg.ivf_ann.FaissIvfFlat.train(m, nlist, x[:2000], niter=3, seed=7)
    ix = sq.FaissIvfSq8.train(m, nlist, x[:2000], niter=3, seed=7)
    assert ix.centroids().tobytes() == flat.centroids().tobytes()
    for index in (flat, ix):
        index.add(x[:1234], ids[:1234])
        index.add(x[1234:], ids[1234:])
    assert ix.n == n
    assert np.array_equal(ix.assignment()[0], ids) and np.array_equal(ix.assignment()[1], flat.assignment()[1])
    assert np.array_equal(ix.list_sizes(), flat.list_sizes())
    flat.search(q, 10, 5)
    ix.search(q, 10, 5)
    assert ix.last_probes().tobytes() == flat.last_probes().tobytes()
    assert ix.last_stats()["rows_scanned"] == flat.last_stats()["rows_scanned"] > 0
    with pytest.raises(sq.IvfSqError, match="ids"):
        ix.add(x[:4])
    flat.close()
    ix.close()


# ---- the scan -----------------------------------------------------------------------------------------------------------
N_SCAN, NLIST_SCAN, NQ_SCAN = 6000, 16, 32


@pytest.fixture(scope="module")
def scan_case(pkg, sq):
    """(the SQ8 index, its Flat twin, the queries) per (d, metric): 6000 standard-normal rows under permuted, scaled ids;
    16 centroids given, the last a copy of the first -- every tie goes to the lower cell, so cell 15 receives nothing and is
    probed all the same.  The ranges are those of the rows."""
    built = {}

    def get(d, metric):
        if (d, metric) not in built:
            m = _metric(pkg, metric)
            rng = np.random.default_rng(1000 + d)
            x = rng.standard_normal((N_SCAN, d)).astype(np.float32)
            ids = rng.permutation(N_SCAN).astype(np.int64) * 7 + 1
            cent = x[rng.choice(N_SCAN, NLIST_SCAN, replace=False)].copy()
            cent[NLIST_SCAN - 1] = cent[0]
            vmin, vdiff = ref.ranges(ref.prepare(int(m), x))
            ix = sq.FaissIvfSq8.load(m, cent, vmin, vdiff)
            flat = pkg.ivf_ann.FaissIvfFlat.load(m, cent)
            ix.add(x, ids)
            flat.add(x, ids)
            assert ix.list_sizes()[NLIST_SCAN - 1] == 0 and ix.list_sizes().sum() == N_SCAN
            built[(d, metric)] = (ix, flat, rng.standard_normal((NQ_SCAN, d)).astype(np.float32))
        return built[(d, metric)]

    yield get
    for ix, flat, _ in built.values():
        ix.close()
        flat.close()


@pytest.mark.parametrize("k,nprobe", [(1, 1), (10, 3), (100, 16), (1024, 16)])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [16, 48, 272, 512])
def test_scan_against_the_restatement(pkg, scan_case, d, metric, k, nprobe):
    ix, _, q = scan_case(d, metric)
    # k = 1024: distances concentrate, the share of unclear positions has no cap; positions and distances are all checked
    _check_search(ix, _metric(pkg, metric), q, k, nprobe, cap=0.20 if k <= 100 else None)
    stats = ix.last_stats()
    assert stats["rounds"] == 1 and stats["rows_scanned"] == int(ix.list_sizes()[ix.last_probes()].sum())


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [16, 48, 272, 512])
def test_recall_of_the_flat_twins_answer(pkg, scan_case, d, metric):
    ix, flat, q = scan_case(d, metric)
    for nprobe in (3, 16):
        f_ids, _, f_cnt = flat.search(q, 10, nprobe)
        s_ids, _, s_cnt = ix.search(q, 10, nprobe)
        assert np.array_equal(ix.last_probes(), flat.last_probes()) and np.array_equal(f_cnt, s_cnt) and (f_cnt == 10).all()
        share = np.mean([len(set(f_ids[i].tolist()) & set(s_ids[i].tolist())) / 10 for i in range(len(q))])
        print(f"d {d} {metric} nprobe {nprobe}: share of the flat top-10 in the SQ8 top-10 {share:.3f}")
        assert share >= 0.90


# ---- block edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("twice", [False, True])
@pytest.mark.parametrize("sizes", [(0, 1, 31, 32), (33, 65, 0, 1)])
def test_block_edges(pkg, sq, sizes, twice):
    """Four cells whose lists hold 0, 1, 31, 32, 33 and 65 rows over the two builds; `twice`: every row is there a second
    time under another id (the lists are twice as long: 2, 62, 64, 66 and 130)."""
    m = _metric(pkg, "L2")
    d = 64
    rng = np.random.default_rng(sum(sizes) + twice)
    cent = np.zeros((4, d), np.float32)
    cent[np.arange(4), np.arange(4)] = 10.0
    x = np.concatenate([cent[c] + 0.5 * rng.standard_normal((s, d)).astype(np.float32) for c, s in enumerate(sizes)])
    n = len(x)
    ids = rng.permutation(n).astype(np.int64) + 100
    vmin, vdiff = ref.ranges(ref.prepare(int(m), x))
    ix = sq.FaissIvfSq8.load(m, cent, vmin, vdiff)
    ix.add(x, ids)
    if twice:
        ix.add(x, ids + 1000)
    mult = 2 if twice else 1
    assert ix.list_sizes().tolist() == [mult * s for s in sizes]
    valid = set(ids.tolist()) | (set((ids + 1000).tolist()) if twice else set())
    q = (cent + 0.1 * rng.standard_normal((4, d))).astype(np.float32)
    for k, nprobe in ((1, 1), (40, 1), (300, 4), (64, 2)):
        got_ids, got_dist, cnt = _check_search(ix, m, q, k, nprobe)
        probes = ix.last_probes()
        for c in range(4):
            assert probes[c, 0] == c
            assert cnt[c] == min(k, mult * sum(sizes[p] for p in probes[c])), "a padding slot is never returned"
            assert set(got_ids[c, :cnt[c]].tolist()) <= valid
        if nprobe == 1:
            assert cnt[sizes.index(0)] == 0, "a query that probes only an empty list"
        if twice and k == 300:
            # everything probed came back: a row and its copy are neighbours, equal distance, the lower id first
            for c in range(4):
                pos = {i: p for p, i in enumerate(got_ids[c, :cnt[c]].tolist())}
                for i in ids.tolist():
                    assert pos[i + 1000] == pos[i] + 1 and got_dist[c, pos[i]] == got_dist[c, pos[i] + 1]
    ix.close()


# ---- groups -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [33, 70])
def test_many_queries_probe_one_cell(pkg, sq, nq):
    m = _metric(pkg, "InnerProduct")
    rng = np.random.default_rng(nq)
    d = 48
    cent = (4.0 * np.eye(3, d)).astype(np.float32)
    x = np.concatenate([cent[c] + rng.standard_normal((300 + 7 * c, d)).astype(np.float32) for c in range(3)])
    vmin, vdiff = ref.ranges(ref.prepare(int(m), x))
    ix = sq.FaissIvfSq8.load(m, cent, vmin, vdiff)
    ix.add(x)
    q = (cent[1] + 0.2 * rng.standard_normal((nq, d))).astype(np.float32)
    _check_search(ix, m, q, 20, 1)
    assert (ix.last_probes() == 1).all(), "all queries probe one cell: two and three groups of at most 32"
    assert ix.last_stats()["rows_scanned"] == nq * int(ix.list_sizes()[1]) > nq * 250
    ix.close()


@pytest.mark.parametrize("nq", [1, 4097])
def test_one_query_and_more_than_a_chunk(pkg, sq, nq):
    m = _metric(pkg, "L2")
    rng = np.random.default_rng(nq)
    n, d = 5000, 16
    x = rng.standard_normal((n, d)).astype(np.float32)
    ix = sq.FaissIvfSq8.train(m, 8, x, niter=2, seed=3)
    ix.add(x, np.arange(n, dtype=np.int64)[::-1] * 2)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    _check_search(ix, m, q, 5, 2)
    assert ix.last_probes().shape == (nq, 2)
    ix.close()


# ---- the fallback round -------------------------------------------------------------------------------------------------
def test_fallback_round(pkg, sq):
    m = _metric(pkg, "L2")
    rng = np.random.default_rng(77)
    n, d = 9000, 32
    x = rng.standard_normal((n, d)).astype(np.float32)
    vmin, vdiff = ref.ranges(ref.prepare(int(m), x))
    ix = sq.FaissIvfSq8.load(m, np.zeros((1, d), np.float32), vmin, vdiff)
    ix.add(x, rng.permutation(n).astype(np.int64))
    _check_search(ix, m, rng.standard_normal((3, d)).astype(np.float32), 1024, 1)
    assert ix.last_stats()["rounds"] >= 2, "9000 rows overflow the survivor buffer of 8192"
    ix.close()


# ---- determinism --------------------------------------------------------------------------------------------------------
def test_determinism(pkg, sq):
    m = _metric(pkg, "Cosine")
    rng = np.random.default_rng(8)
    n, d = 4000, 48
    x = rng.standard_normal((n, d)).astype(np.float32)
    ids = rng.permutation(n).astype(np.int64) * 3
    q = rng.standard_normal((40, d)).astype(np.float32)

    def build(parts):
        ix = sq.FaissIvfSq8.train(m, 12, x[:1500], niter=3, seed=4)
        for lo, hi in parts:
            ix.add(x[lo:hi], ids[lo:hi])
        return ix

    def exports(ix):
        return [a.tobytes() for a in (ix.centroids(), *ix.ranges(), ix.codes(), *ix.assignment(), ix.list_sizes())]

    def answer(ix):
        return [a.tobytes() for a in ix.search(q, 50, 4)]

    a, b, c = build([(0, n)]), build([(0, n)]), build([(0, 1700), (1700, n)])
    assert exports(a) == exports(b), "two trainings and builds export identical bytes"
    first = answer(a)
    assert answer(a) == first, "a search repeated"
    assert answer(b) == first
    assert exports(c) == exports(a) and answer(c) == first, "two adds answer as one add of the same rows"
    for ix in (a, b, c):
        ix.close()
