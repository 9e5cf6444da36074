"""IVF-Flat on the device (include/ivf_ann.h) against the float64 restatement tests/_ivf_ref.py, fed with what the index
exports (centroids, assignment, probes) -- never with the device's own answers.  Tolerance: the project's 1e-5 / 1e-5 on
distances (tests/test_dense_gpu.py); ids and cells must agree wherever the restatement's distances are further apart than
that.  PARITY UNPINNED against Faiss (not vendored in the reference), as the header says."""
import importlib.util
import os

import numpy as np
import pytest

import _ivf_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = ref.RTOL, ref.ATOL
METRICS = ["L2", "Cosine", "InnerProduct"]


def _metric(pkg, name):
    return getattr(pkg.dense_ann.DistanceMetric, name)


def _clustered(rng, n, d, n_clusters, sigma):
    centres = rng.standard_normal((n_clusters, d)).astype(np.float32)
    return (centres[rng.integers(0, n_clusters, n)] + sigma * rng.standard_normal((n, d))).astype(np.float32)


def _close(got, want):
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


def _check_cells(metric, prepared, centroids, got_cells, nprobe=1):
    """got_cells [m, nprobe] against the nprobe nearest centroids: distances everywhere, cells at clear positions.
    Returns the share of unclear positions."""
    want, dist = ref.probe(int(metric), prepared, centroids, nprobe)
    got_cells = np.asarray(got_cells).reshape(len(prepared), -1)
    assert got_cells.shape == want.shape
    unclear = 0
    for i in range(len(prepared)):
        order = np.lexsort((np.arange(dist.shape[1]), dist[i]))
        r_dist = dist[i, order[:want.shape[1]]]
        nxt = dist[i, order[want.shape[1]]] if dist.shape[1] > want.shape[1] else np.inf
        _close(dist[i, got_cells[i]], r_dist)
        clear = ref.clear_positions(r_dist, nxt)
        assert np.array_equal(got_cells[i][clear], want[i][clear])
        assert len(set(got_cells[i].tolist())) == got_cells.shape[1]
        unclear += int((~clear).sum())
    return unclear / want.size


def _check_search(ix, metric, prepared_rows, queries, k, nprobe, got=None):
    """The device's answer against the exhaustive top-k over the union of the lists of the cells it reported."""
    got_ids, got_dist, cnt = ix.search(queries, k, nprobe) if got is None else got
    probes = ix.last_probes()
    ids, cells = ix.assignment()
    want = ref.search_probed(int(metric), prepared_rows, ids, cells, probes, ref.prepare(int(metric), queries), k)
    for q, (r_ids, r_dist, nxt) in enumerate(want):
        m = len(r_ids)
        assert cnt[q] == m, f"query {q}: count {cnt[q]} != {m}"
        _close(got_dist[q, :m], r_dist)
        clear = ref.clear_positions(r_dist, nxt)
        assert np.array_equal(got_ids[q, :m][clear], r_ids[clear])
        assert len(set(got_ids[q, :m].tolist())) == m, "no id twice"
    return got_ids, got_dist, cnt, want


def _rows_scanned(ix):
    sizes = ix.list_sizes()
    return int(sizes[ix.last_probes()].sum())


# ---- 4. structure -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_structure_after_two_adds(pkg, metric):
    m = _metric(pkg, metric)
    rng = np.random.default_rng(4)
    n, d, nlist = 50000, 64, 256
    x = rng.standard_normal((n, d)).astype(np.float32)
    ids = (rng.permutation(n).astype(np.int64) * 3 + 11)
    ix = pkg.ivf_ann.FaissIvfFlat.load(m, x[rng.choice(n, nlist, replace=False)])
    ix.add(x[:20000], ids[:20000])
    ix.add(x[20000:], ids[20000:])
    assert ix.n == n
    sizes = ix.list_sizes()
    got_ids, cells = ix.assignment()
    assert sizes.sum() == n and np.array_equal(got_ids, ids)
    assert np.array_equal(sizes, np.bincount(cells, minlength=nlist))
    print("list sizes", sizes.min(), "..", sizes.max())
    centroids = ix.centroids()
    assert np.array_equal(centroids, ref.prepare(int(m), centroids)), "stored centroids are fp16 values"
    unclear = _check_cells(m, ref.prepare(int(m), x), centroids, cells)
    print("unclear assignments", unclear)
    # the ids rule, both ways
    with pytest.raises(pkg.ivf_ann.IvfError, match="ids"):
        ix.add(x[:4])
    ix.close()
    ix = pkg.ivf_ann.FaissIvfFlat.load(m, x[:nlist])
    ix.add(x[:100])
    with pytest.raises(pkg.ivf_ann.IvfError, match="ids"):
        ix.add(x[:4], ids[:4])
    assert np.array_equal(ix.assignment()[0], np.arange(100))
    ix.close()


# ---- 5. probing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,nlist,nprobe,clustered", [(64, 64, 8, False), (256, 256, 16, False), (64, 64, 8, True)])
def test_probes_are_the_nearest_cells(pkg, metric, d, nlist, nprobe, clustered):
    m = _metric(pkg, metric)
    rng = np.random.default_rng(5 + d)
    n = 20000
    x = _clustered(rng, n, d, nlist // 4, 0.5) if clustered else rng.standard_normal((n, d)).astype(np.float32)
    ix = pkg.ivf_ann.FaissIvfFlat.train(m, nlist, x, niter=5, seed=3)
    ix.add(x)
    q = (x[rng.choice(n, 1024)] + 0.3 * rng.standard_normal((1024, d))).astype(np.float32) if clustered else \
        rng.standard_normal((1024, d)).astype(np.float32)
    ix.search(q, 10, nprobe)
    probes = ix.last_probes()
    assert probes.shape == (1024, nprobe)
    unclear = _check_cells(m, ref.prepare(int(m), q), ix.centroids(), probes, nprobe)
    print(f"unclear probe positions: {unclear:.4f}")
    assert unclear <= 0.10, "more than 10% of the probe positions unclear: the comparison would be vacuous"
    assert ix.last_stats()["rows_scanned"] == _rows_scanned(ix)
    ix.close()


# ---- 6. scan exactness --------------------------------------------------------------------------------------------
_CACHE = {}


@pytest.fixture(scope="module")
def scan_setup(pkg):
    def get(metric, d):
        key = (metric, d)
        if key not in _CACHE:
            m = _metric(pkg, metric)
            rng = np.random.default_rng(60 + d)
            n, nlist = 20000, 64
            x = rng.standard_normal((n, d)).astype(np.float32)
            ids = rng.permutation(n).astype(np.int64) * 5 + 2
            cent = x[rng.choice(n, nlist, replace=False)].copy()
            # one cell nothing falls into: far away for L2; the zero vector never has the largest dot product
            cent[7] = 100.0 if metric == "L2" else 0.0
            ix = pkg.ivf_ann.FaissIvfFlat.load(m, cent)
            ix.add(x, ids)
            dense = pkg.dense_ann.BruteForceIndex.build(m, x, ids)
            q = rng.standard_normal((48, d)).astype(np.float32)
            _CACHE[key] = (m, ix, dense, ref.prepare(int(m), x), q, nlist)
        return _CACHE[key]

    yield get
    for _, ix, dense, *_ in _CACHE.values():
        ix.close()
        dense.close()
    _CACHE.clear()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("k", [1, 10, 200, 1024])
@pytest.mark.parametrize("nprobe", [1, 8, 64])
def test_scan_is_exact_over_the_probed_lists(pkg, scan_setup, metric, d, k, nprobe):
    m, ix, dense, prepared, q, nlist = scan_setup(metric, d)
    assert ix.list_sizes()[7] == 0, "the empty list"
    got_ids, got_dist, cnt, want = _check_search(ix, m, prepared, q, k, nprobe)
    assert ix.last_stats()["rows_scanned"] == _rows_scanned(ix)
    if nprobe == nlist:  # every list probed: the exhaustive index's answer, to the same rule
        d_ids, d_dist, d_cnt = dense.search(q, k)
        assert np.array_equal(cnt, d_cnt)
        for qi, (r_ids, r_dist, nxt) in enumerate(want):
            _close(d_dist[qi, :cnt[qi]], r_dist)
            _close(got_dist[qi, :cnt[qi]], d_dist[qi, :cnt[qi]])
            clear = ref.clear_positions(r_dist, nxt)
            assert np.array_equal(got_ids[qi, :cnt[qi]][clear], d_ids[qi, :cnt[qi]][clear])


@pytest.mark.parametrize("metric", METRICS)
def test_lists_of_size_zero_and_one_fewer_rows_than_k_and_duplicates(pkg, metric):
    m = _metric(pkg, metric)
    rng = np.random.default_rng(61)
    d = 64
    cent = np.zeros((4, d), np.float32)
    for c in range(4):
        cent[c, c] = 1.0
    base = (rng.standard_normal((30, d)) * 0.05).astype(np.float16).astype(np.float32)
    base[:, 0] += 1.0                      # 30 rows near centroid 0
    one = np.zeros((1, d), np.float32)
    one[0, 1] = 1.0                        # one row on centroid 1; cells 2 and 3 stay empty
    x = np.concatenate([base, base, one])  # every row of cell 0 twice, under different ids
    ids = np.concatenate([np.arange(100, 130), np.arange(30), [999]]).astype(np.int64)
    ix = pkg.ivf_ann.FaissIvfFlat.load(m, cent)
    ix.add(x, ids)
    assert ix.list_sizes().tolist() == [60, 1, 0, 0]
    q = np.concatenate([cent, base[:3] + 0.01]).astype(np.float32)
    prepared = ref.prepare(int(m), x)
    for k, nprobe in [(1, 1), (10, 1), (100, 1), (100, 2), (1024, 4)]:
        got_ids, got_dist, cnt, _ = _check_search(ix, m, prepared, q, k, nprobe)
        assert cnt[1] == min(k, 1 if nprobe == 1 else 61) and cnt[0] == min(k, 60 if nprobe == 1 else 61)
        if nprobe == 1:
            assert cnt[2] == 0 and cnt[3] == 0, "a query that probes an empty list alone"
        # duplicates: equal distance, the lower id first
        pairs = got_ids[4, :min(k, 60) // 2 * 2].reshape(-1, 2)
        assert np.all(pairs[:, 0] + 100 == pairs[:, 1])
    ix.close()


def test_a_cell_larger_than_the_survivor_buffer_takes_the_fallback_round(pkg):
    m = _metric(pkg, "L2")
    rng = np.random.default_rng(62)
    d = 64
    cent = np.zeros((8, d), np.float32)
    cent[1:] = 20.0 * rng.standard_normal((7, d))
    x = np.concatenate([rng.standard_normal((9000, d)), cent[1:] + rng.standard_normal((7, d))]).astype(np.float32)
    ix = pkg.ivf_ann.FaissIvfFlat.load(m, cent)
    ix.add(x)
    assert ix.list_sizes()[0] >= 9000 > 8192
    q = rng.standard_normal((40, d)).astype(np.float32)
    _check_search(ix, m, ref.prepare(int(m), x), q, 1024, 1)
    st = ix.last_stats()
    print(st)
    assert st["rounds"] >= 2, "the fallback round fired"
    assert st["rows_scanned"] == _rows_scanned(ix)
    _check_search(ix, m, ref.prepare(int(m), x), q, 10, 8)
    ix.close()


@pytest.mark.parametrize("nq", [1, 4097])
def test_one_query_and_the_chunk_boundary_of_the_coarse_search(pkg, nq):
    m = _metric(pkg, "InnerProduct")
    rng = np.random.default_rng(63)
    n, d = 5000, 64
    x = rng.standard_normal((n, d)).astype(np.float32)
    ix = pkg.ivf_ann.FaissIvfFlat.load(m, x[:16])
    ix.add(x)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    _check_search(ix, m, ref.prepare(int(m), x), q, 10, 4)
    assert ix.last_probes().shape == (nq, 4)
    assert ix.last_stats()["rows_scanned"] == _rows_scanned(ix)
    ix.close()


# ---- 8. determinism -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_determinism(pkg, metric):
    m = _metric(pkg, metric)
    rng = np.random.default_rng(8)
    n, d, nlist = 20000, 64, 64
    x = _clustered(rng, n, d, 16, 0.7)
    a = pkg.ivf_ann.FaissIvfFlat.train(m, nlist, x[:8000], niter=4, seed=9)
    b = pkg.ivf_ann.FaissIvfFlat.train(m, nlist, x[:8000], niter=4, seed=9)
    assert a.centroids().tobytes() == b.centroids().tobytes()
    c = pkg.ivf_ann.FaissIvfFlat.train(m, nlist, x[:8000], niter=4, seed=10)
    assert a.centroids().tobytes() != c.centroids().tobytes(), "the seed picks the initial centroids"
    c.close()
    a.add(x[:12000])
    a.add(x[12000:])
    b.add(x)
    q = rng.standard_normal((100, d)).astype(np.float32)
    for k, nprobe in [(10, 4), (200, 16)]:
        r1 = a.search(q, k, nprobe)
        r2 = a.search(q, k, nprobe)
        r3 = b.search(q, k, nprobe)
        for u, v, w in zip(r1, r2, r3):
            assert u.tobytes() == v.tobytes(), "search twice"
            assert u.tobytes() == w.tobytes(), "add(X0); add(X1) against add(X0 ++ X1)"
    a.close()
    b.close()


# ---- 9. training --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_training_lowers_the_objective(pkg, metric):
    m = _metric(pkg, metric)
    rng = np.random.default_rng(9)
    n, d, nlist = 20000, 64, 64
    x = _clustered(rng, n, d, nlist // 4, 0.7)
    prepared = ref.prepare(int(m), x)
    obj = {}
    for niter in (-1, 1, 10):
        ix = pkg.ivf_ann.FaissIvfFlat.train(m, nlist, x, niter=niter, seed=5)
        cent = ix.centroids()
        if m != pkg.dense_ann.DistanceMetric.L2:
            np.testing.assert_allclose(np.linalg.norm(cent.astype(np.float64), axis=1), 1.0, atol=2e-3)
        obj[niter] = ref.objective(int(m), prepared, cent)
        ix.close()
    print("objective", obj)
    # Lloyd's monotonicity; 1e-5 relative for the fp16 rounding of the stored centroids
    assert obj[1] <= obj[-1] + 1e-5 * abs(obj[-1])
    assert obj[10] <= obj[1] + 1e-5 * abs(obj[1])


# ---- 10. recall ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_recall_grows_with_nprobe_and_is_complete_at_nlist(pkg, metric):
    m = _metric(pkg, metric)
    rng = np.random.default_rng(10)
    n, d, nlist, k = 30000, 64, 64, 10
    x = _clustered(rng, n, d, nlist // 4, 1.0)
    ix = pkg.ivf_ann.FaissIvfFlat.train(m, nlist, x[:10000], niter=5, seed=2)
    ix.add(x)
    dense = pkg.dense_ann.BruteForceIndex.build(m, x)
    q = (x[rng.choice(n, 256)] + rng.standard_normal((256, d))).astype(np.float32)
    t_ids, t_dist, _ = dense.search(q, k)
    recalls = []
    for nprobe in (1, 8, 32, nlist):
        ids, dist, cnt = ix.search(q, k, nprobe)
        recalls.append(float(np.mean([len(set(ids[i, :cnt[i]].tolist()) & set(t_ids[i].tolist())) / k for i in range(len(q))])))
    print("recall@10 at nprobe 1, 8, 32, nlist:", recalls)
    assert all(b >= a for a, b in zip(recalls, recalls[1:])), recalls
    _close(dist, t_dist)
    for i in range(len(q)):
        clear = ref.clear_positions(t_dist[i].astype(np.float64), np.inf)
        clear[-1] = False
        assert np.array_equal(ids[i][clear], t_ids[i][clear])
    assert recalls[-1] >= 1.0 - (1.0 / k), "complete up to swaps at unclear positions"
    ix.close()
    dense.close()


def test_flat_index_answers_as_before_the_shared_core(pkg):
    """FaissIvfFlat over two adds with ids: both searches with their probes, list_sizes() and assignment(), byte for byte
    against what the library gave before ivf_ann.hip and ivfpq_ann.hip shared csrc/ivf_core.h
    (tests/golden/ivf_family_baseline.npz, written by make_ivf_family_baseline.py)."""
    path = os.path.join(ROOT, "tests", "golden", "make_ivf_family_baseline.py")
    spec = importlib.util.spec_from_file_location("make_ivf_family_baseline", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    base = np.load(os.path.join(ROOT, "tests", "golden", "ivf_family_baseline.npz"))
    want = {n: base[n] for n in base.files if n.startswith("flat_")}
    got = gen.flat_answers(pkg)
    assert sorted(got) == sorted(want) and len(got) == len(gen.METRICS) * (4 * len(gen.SEARCHES) + 3)
    for name in sorted(got):
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), name
    assert any(want[n].any() for n in want if n.endswith("_dist"))
