"""IVF-PQ on the device (include/ivfpq_ann.h) against the restatement tests/_ivfpq_ref.py, fed with what the index exports
(centroids, codebooks, codes, assignment, probes) -- never with the device's own distances.

Tolerance: the project's 1e-5 / 1e-5, widened by the fp32 bound of the arithmetic, (M + dsub + d + 4) 2^-24 S, where S is the
float64 sum of the absolute elementary products (InnerProduct / Cosine) or of the squared terms (L2); L2 is compared in the
squared domain with 2^-22 s more for the fp32 square root.  Ids and codes must agree wherever the restatement's neighbours
are more than twice that apart; no more than 15 % of the positions of a test may be left out that way.
PARITY UNPINNED against Faiss's training and encoding (not vendored in the reference), as the header says.

Inputs of the searches with k up to 1024 (scan parity, the fallback round): rows whose distances do not crowd.  Of rows with
independent N(0,1) components the distances to a query concentrate: their relative spread is about sqrt(2 / d), while the
tolerance is about 3e-5 relative at d = 256, so among a few hundred candidates neighbouring values already lie within twice
the tolerance of each other.  Computed from the restatement alone (no device involved), N(0,1) rows, nlist = 64, the share
of unclear positions at (k, nprobe) = (200, 8) and (1024, 64) is 0.23 and 0.67 for L2 256/64 at n = 6000, 0.28 and 0.74 at
n = 20000, and up to 0.88 for Cosine: no comparison of ids would be left.  Those searches therefore take N(0,1) latent
rows of dimension 3 under a random N(0,1) linear map into R^d, plus 0.3 N(0,1) in every component (_low_dimensional): the
in-plane part spreads the distances (Cosine: nearly uniformly over [0, 2]) and the noise keeps the code tuples of a cell
distinct.  Even then 1024 values within [0, 2] at a tolerance of 3.3e-5 bound the candidates of the k = 1024, nprobe =
nlist search to about 2000, hence n = 1500 in the scan-parity test; the restatement alone puts its worst case (Cosine /
InnerProduct 256/64, k = 1024, nprobe = 64) at 0.12 unclear, every other at less.  Long lists (several blocks of 64 rows,
9000 rows in one cell) are what the structure, determinism, recall and fallback-round tests hold."""
import numpy as np
import pytest

import _ivfpq_ref as ref

pytestmark = pytest.mark.gpu

METRICS = ["L2", "Cosine", "InnerProduct"]
MAX_UNCLEAR = 0.15


def _metric(pkg, name):
    return getattr(pkg.dense_ann.DistanceMetric, name)


def _clustered(rng, n, d, n_clusters, sigma):
    centres = rng.standard_normal((n_clusters, d)).astype(np.float32)
    return (centres[rng.integers(0, n_clusters, n)] + sigma * rng.standard_normal((n, d))).astype(np.float32)


def _low_dimensional(rng, n, d, r=3, eps=0.3):
    """N(0,1) latent rows of dimension r under a random N(0,1) / sqrt(r) linear map into R^d, plus eps N(0,1) per component:
    distances that spread instead of concentrating (see the module's docstring)."""
    basis = rng.standard_normal((r, d)) / np.sqrt(r)
    return (rng.standard_normal((n, r)) @ basis + eps * rng.standard_normal((n, d))).astype(np.float32)


def _grid_codebooks(rng, M, dsub, step):
    """Distinct codewords whose entries are small multiples of `step` (a power of two: fp16-exact): the first entry of
    codeword j is one of 256 distinct values in [-128 step, 128 step), the others lie within 32 steps of zero."""
    cb = rng.integers(-32, 33, (M, 256, dsub)).astype(np.float64)
    for m in range(M):
        cb[m, :, 0] = rng.permutation(256) - 128
    return (cb * step).astype(np.float32)


def _want(ix, metric, queries, kmax):
    """The restatement's answer over what the index exports for its last search."""
    ids, cells = ix.assignment()
    return ref.adc_search(int(metric), ix.centroids(), ix.codebooks(), ix.codes(), ids, cells, ix.last_probes(),
                          ref.prepare(int(metric), queries), kmax)


def _compare(ix, metric, got, want, k):
    """got = (ids, dist, cnt) of a search with this k against want (from _want with kmax >= k).  Returns (unclear, total)."""
    got_ids, got_dist, cnt = got
    M, dsub = ix.M, ix.d // ix.M
    unclear = total = 0
    for q, (r_ids, r_val, r_s) in enumerate(want):
        m = min(k, len(r_ids))
        assert cnt[q] == m, f"query {q}: count {cnt[q]} != {m}"
        if m == 0:
            continue
        tol = ref.tolerance(int(metric), r_val, r_s, M, dsub)
        g = got_dist[q, :m].astype(np.float64)
        g = g * g if int(metric) == ref.L2 else g
        err = np.abs(g - r_val[:m])
        assert np.all(err <= tol[:m]), f"query {q}: error {err.max()} against tolerance {tol[:m][err.argmax()]}"
        assert np.all(np.diff(got_dist[q, :m]) >= 0), "ascending"
        nxt = r_val[m] if len(r_val) > m else np.inf
        clear = ref.clear_positions(r_val[:m], nxt, tol[:m])
        assert np.array_equal(got_ids[q, :m][clear], r_ids[:m][clear])
        assert len(set(got_ids[q, :m].tolist())) == m, "no id twice"
        unclear += int((~clear).sum())
        total += m
    return unclear, total


def _check_search(ix, metric, queries, k, nprobe, max_unclear=MAX_UNCLEAR):
    got = ix.search(queries, k, nprobe)
    unclear, total = _compare(ix, metric, got, _want(ix, metric, queries, k), k)
    share = unclear / max(total, 1)
    print(f"k={k} nprobe={nprobe}: unclear positions {share:.4f} of {total}")
    assert share <= max_unclear, "too many positions unclear: the comparison would be vacuous"
    return got


def _rows_scanned(ix):
    return int(ix.list_sizes()[ix.last_probes()].sum())


def _check_codes(ix, metric, x):
    """codes() against the restatement's encoding of the exported centroids and codebooks.  Returns the unclear share."""
    M, dsub = ix.M, ix.d // ix.M
    _, cells = ix.assignment()
    res = ref.residuals(ref.prepare(int(metric), x), ix.centroids(), cells)
    got = ix.codes()
    want, best, second, at_got = ref.encode(res, ix.codebooks(), got)
    tol = ref.ATOL + ref.RTOL * best + ref.fp32_bound(M, dsub) * best
    assert np.all(at_got - best <= tol), "the encoded codeword is within tolerance of the nearest"
    clear = second - best > 2 * tol
    assert np.array_equal(got[clear], want[clear])
    return float((~clear).mean())


# ---- 1. exactly representable rows ----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,M", [(16, 4), (64, 16)])
def test_exactly_representable_rows(pkg, metric, d, M):
    m = _metric(pkg, metric)
    rng = np.random.default_rng(100 + d)
    dsub, nlist, n = d // M, 8, 3000
    # centroids far apart on distinct axes, small codewords: a row centroid[c] + codewords lies well inside cell c
    cent = np.zeros((nlist, d), np.float32)
    for c in range(nlist):
        cent[c, c] = 1.0 if metric == "Cosine" else 16.0
    cb = _grid_codebooks(rng, M, dsub, 1 / 64 if metric != "Cosine" else 1 / 1024)
    codes = rng.integers(0, 256, (n, M))
    cells = rng.integers(0, nlist, n)
    x = (cent[cells] + np.concatenate([cb[j, codes[:, j]] for j in range(M)], axis=1)).astype(np.float32)
    ids = rng.permutation(n).astype(np.int64) * 7 + 3
    ix = pkg.ivfpq_ann.FaissIvfPq.load(m, cent, cb)
    assert np.array_equal(ix.codebooks(), cb) and ix.M == M
    ix.add(x, ids)
    assert np.array_equal(ix.assignment()[1], cells)
    if metric != "Cosine":  # (Cosine rows are normalised first: their residuals are no longer the codewords)
        assert np.array_equal(x.astype(np.float16).astype(np.float32), x), "rows are fp16-exact"
        assert np.array_equal(ix.codes(), codes), "exported codes are the constructing codes"
    else:
        assert _check_codes(ix, m, x) <= MAX_UNCLEAR
    q = (x[rng.choice(n, 32)] + 0.05 * rng.standard_normal((32, d))).astype(np.float32)
    got_ids, got_dist, cnt = _check_search(ix, m, q, 10, 3)
    if metric != "Cosine":
        # the codes reconstruct the rows exactly: the distances are those to the rows themselves
        order = np.argsort(ids)
        rows = x[order][np.searchsorted(ids[order], got_ids)].astype(np.float64)
        qp = ref.prepare(int(m), q).astype(np.float64)
        if metric == "L2":
            exact = ((rows - qp[:, None, :]) ** 2).sum(axis=2)
            got = got_dist.astype(np.float64) ** 2
            S = exact
        else:
            exact = 1.0 - (rows * qp[:, None, :]).sum(axis=2)
            got = got_dist.astype(np.float64)
            S = np.abs(rows * qp[:, None, :]).sum(axis=2)
        assert np.all(cnt == 10)
        assert np.all(np.abs(got - exact) <= ref.tolerance(int(m), exact, S, M, dsub))
    ix.close()


# ---- 2. structure -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_structure_after_two_adds(pkg, metric):
    m = _metric(pkg, metric)
    rng = np.random.default_rng(4)
    n, d, M, nlist = 20000, 64, 8, 64
    x = rng.standard_normal((n, d)).astype(np.float32)
    ids = (rng.permutation(n).astype(np.int64) * 3 + 11)
    ix = pkg.ivfpq_ann.FaissIvfPq.train(m, nlist, M, x[:8000], niter=2, seed=4)
    ix.add(x[:7000], ids[:7000])
    ix.add(x[7000:], ids[7000:])
    assert ix.n == n
    sizes = ix.list_sizes()
    got_ids, cells = ix.assignment()
    assert sizes.sum() == n and np.array_equal(got_ids, ids)
    assert np.array_equal(sizes, np.bincount(cells, minlength=nlist))
    centroids = ix.centroids()
    assert np.array_equal(centroids, centroids.astype(np.float16).astype(np.float32)), "stored centroids are fp16 values"
    # assignment: the nearest centroid, wherever the restatement's two nearest are further apart than the tolerance
    want_cells, dist = ref.assign(int(m), ref.prepare(int(m), x), centroids)
    part = np.partition(dist, 1, axis=1)
    clear = part[:, 1] - part[:, 0] > 2 * (ref.ATOL + ref.RTOL * np.abs(part[:, 0]))
    assert np.array_equal(cells[clear], want_cells[clear]) and clear.mean() >= 1 - MAX_UNCLEAR
    assert ix.codes().shape == (n, M)
    unclear = _check_codes(ix, m, x)
    print("unclear codes", unclear)
    assert unclear <= MAX_UNCLEAR
    # the ids rule, both ways
    with pytest.raises(pkg.ivfpq_ann.IvfPqError, match="ids"):
        ix.add(x[:4])
    assert ix.n == n
    cent, cb = ix.centroids(), ix.codebooks()
    ix.close()
    ix = pkg.ivfpq_ann.FaissIvfPq.load(m, cent, cb)
    ix.add(x[:100])
    with pytest.raises(pkg.ivfpq_ann.IvfPqError, match="ids"):
        ix.add(x[:4], ids[:4])
    assert np.array_equal(ix.assignment()[0], np.arange(100))
    ix.close()


# ---- 3. scan parity ---------------------------------------------------------------------------------------------------
_CACHE = {}
_WANT = {}


@pytest.fixture(scope="module")
def scan_setup(pkg):
    def get(metric, d, M):
        key = (metric, d, M)
        if key not in _CACHE:
            m = _metric(pkg, metric)
            rng = np.random.default_rng(60 + d + M)
            n, nlist = 1500, 64
            x = _low_dimensional(rng, n + 48, d)
            x, q = x[:n], x[n:]
            ids = rng.permutation(n).astype(np.int64) * 5 + 2
            trained = pkg.ivfpq_ann.FaissIvfPq.train(m, nlist, M, x[:1000], niter=-1, seed=6)
            cent = trained.centroids()
            # one cell nothing falls into: far away for L2; the zero vector never has the largest dot product
            cent[7] = 100.0 if metric == "L2" else 0.0
            ix = pkg.ivfpq_ann.FaissIvfPq.load(m, cent, trained.codebooks())
            trained.close()
            ix.add(x, ids)
            _CACHE[key] = (m, ix, q)
        return _CACHE[key]

    yield get
    for _, ix, _ in _CACHE.values():
        ix.close()
    _CACHE.clear()
    _WANT.clear()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,M", [(64, 4), (64, 8), (64, 16), (256, 64), (128, 32)])
@pytest.mark.parametrize("nprobe", [1, 8, 64])
@pytest.mark.parametrize("k", [1, 10, 200, 1024])
def test_scan_matches_the_restatement(pkg, scan_setup, metric, d, M, k, nprobe):
    m, ix, q = scan_setup(metric, d, M)
    assert ix.list_sizes()[7] == 0, "the empty list"
    got = ix.search(q, k, nprobe)
    probes = ix.last_probes()
    key = (metric, d, M, nprobe)
    if key not in _WANT or not np.array_equal(_WANT[key][0], probes):  # one restatement per probe table, shared by the ks
        _WANT[key] = (probes, _want(ix, m, q, 1024))
    unclear, total = _compare(ix, m, got, _WANT[key][1], k)
    print(f"unclear positions {unclear / max(total, 1):.4f} of {total}")
    assert unclear <= MAX_UNCLEAR * total, "the comparison would be vacuous"
    assert ix.last_stats()["rows_scanned"] == _rows_scanned(ix)
    assert ix.last_stats()["rounds"] >= 1


# ---- 4. edge cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_lists_of_size_zero_and_one_fewer_rows_than_k_and_duplicates(pkg, metric):
    m = _metric(pkg, metric)
    rng = np.random.default_rng(61)
    d, M = 64, 8
    cent = np.zeros((4, d), np.float32)
    for c in range(4):
        cent[c, c] = 1.0
    cb = _grid_codebooks(rng, M, d // M, 1 / 1024)
    base = (rng.standard_normal((30, d)) * 0.05).astype(np.float16).astype(np.float32)
    base[:, 0] += 1.0                      # 30 rows near centroid 0
    one = np.zeros((1, d), np.float32)
    one[0, 1] = 1.0                        # one row on centroid 1; cells 2 and 3 stay empty
    x = np.concatenate([base, base, one])  # every row of cell 0 twice, under different ids
    ids = np.concatenate([np.arange(100, 130), np.arange(30), [999]]).astype(np.int64)
    ix = pkg.ivfpq_ann.FaissIvfPq.load(m, cent, cb)
    empty = ix.search(cent, 5, 2)
    assert empty[2].tolist() == [0, 0, 0, 0], "an index without rows answers nothing"
    assert ix.last_stats()["rows_scanned"] == 0 and ix.codes().shape == (0, M)
    ix.add(x, ids)
    assert ix.list_sizes().tolist() == [60, 1, 0, 0]
    codes = ix.codes()
    assert np.array_equal(codes[:30], codes[30:60]), "duplicate rows carry equal codes"
    q = np.concatenate([cent, base[:3] + 0.01]).astype(np.float32)
    for k, nprobe in [(1, 1), (10, 1), (100, 1), (100, 2), (1024, 4)]:
        got_ids, got_dist, cnt = _check_search(ix, m, q, k, nprobe, max_unclear=1.0)  # (every position ties with its duplicate)
        assert cnt[1] == min(k, 1 if nprobe == 1 else 61) and cnt[0] == min(k, 60 if nprobe == 1 else 61)
        if nprobe == 1:
            assert cnt[2] == 0 and cnt[3] == 0, "a query that probes an empty list alone"
        # duplicates: equal distance exactly, the lower id first -- and more generally ascending by (distance, id)
        for qi in range(len(q)):
            c = cnt[qi]
            pairs = list(zip(got_dist[qi, :c].tolist(), got_ids[qi, :c].tolist()))
            assert pairs == sorted(pairs)
        if k >= 2:
            in_cell0 = got_ids[4, :min(k, 60)]
            by_dist = {}
            for i, dd in zip(in_cell0.tolist(), got_dist[4, :min(k, 60)].tolist()):
                by_dist.setdefault(i % 100, set()).add(dd)
            assert all(len(v) == 1 for v in by_dist.values()), "a row and its duplicate tie exactly"
    ix.close()


@pytest.mark.parametrize("nq", [1, 4097])
def test_one_query_and_the_chunk_boundary_of_the_coarse_search(pkg, nq):
    m = _metric(pkg, "InnerProduct")
    rng = np.random.default_rng(63)
    n, d, M = 5000, 64, 8
    x = rng.standard_normal((n, d)).astype(np.float32)
    ix = pkg.ivfpq_ann.FaissIvfPq.train(m, 16, M, x[:1000], niter=1, seed=1)
    ix.add(x)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    got = ix.search(q, 10, 4)
    assert ix.last_probes().shape == (nq, 4)
    assert ix.last_stats()["rows_scanned"] == _rows_scanned(ix)
    # the restatement over the first and the last 40 queries (the last ones lie past the chunk boundary)
    pick = np.unique(np.concatenate([np.arange(min(nq, 40)), np.arange(max(0, nq - 40), nq)]))
    ids, cells = ix.assignment()
    want = ref.adc_search(int(m), ix.centroids(), ix.codebooks(), ix.codes(), ids, cells, ix.last_probes()[pick],
                          ref.prepare(int(m), q[pick]), 10)
    unclear, total = _compare(ix, m, tuple(a[pick] for a in got), want, 10)
    assert unclear <= MAX_UNCLEAR * total
    ix.close()


# ---- 5. the fallback round --------------------------------------------------------------------------------------------
def test_a_cell_larger_than_the_survivor_buffer_takes_the_fallback_round(pkg):
    m = _metric(pkg, "L2")
    rng = np.random.default_rng(62)
    d, M = 64, 16
    cent = np.zeros((8, d), np.float32)
    cent[1:] = 20.0 * rng.standard_normal((7, d))
    body = _low_dimensional(rng, 9040, d)
    x = np.concatenate([body[:9000], cent[1:] + rng.standard_normal((7, d))]).astype(np.float32)
    # codebooks trained on these rows: the residuals scatter over them, no distance is shared by thousands of rows
    trained = pkg.ivfpq_ann.FaissIvfPq.train(m, 8, M, x, niter=2, seed=3)
    ix = pkg.ivfpq_ann.FaissIvfPq.load(m, cent, trained.codebooks())
    trained.close()
    ix.add(x)
    assert ix.list_sizes()[0] >= 9000 > 8192
    q = body[9000:]
    _check_search(ix, m, q, 1024, 1)
    st = ix.last_stats()
    print(st)
    assert st["rounds"] >= 2, "the fallback round fired"
    assert st["rows_scanned"] == _rows_scanned(ix)
    _check_search(ix, m, q, 10, 8)
    ix.close()


# ---- 6. determinism ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_determinism(pkg, metric):
    m = _metric(pkg, metric)
    rng = np.random.default_rng(8)
    n, d, M, nlist = 20000, 64, 8, 64
    x = _clustered(rng, n, d, 16, 0.7)
    a = pkg.ivfpq_ann.FaissIvfPq.train(m, nlist, M, x[:8000], niter=4, seed=9)
    b = pkg.ivfpq_ann.FaissIvfPq.train(m, nlist, M, x[:8000], niter=4, seed=9)
    assert a.centroids().tobytes() == b.centroids().tobytes()
    assert a.codebooks().tobytes() == b.codebooks().tobytes()
    c = pkg.ivfpq_ann.FaissIvfPq.train(m, nlist, M, x[:8000], niter=4, seed=10)
    assert a.codebooks().tobytes() != c.codebooks().tobytes(), "the seed picks the initial codewords"
    c.close()
    a.add(x[:12000])
    a.add(x[12000:])
    b.add(x)
    assert a.codes().tobytes() == b.codes().tobytes(), "codes in the order added"
    assert a.assignment()[0].tobytes() == b.assignment()[0].tobytes()
    q = rng.standard_normal((100, d)).astype(np.float32)
    for k, nprobe in [(10, 4), (200, 16)]:
        r1 = a.search(q, k, nprobe)
        r2 = a.search(q, k, nprobe)
        r3 = b.search(q, k, nprobe)
        for u, v, w in zip(r1, r2, r3):
            assert u.tobytes() == v.tobytes(), "search twice"
            assert u.tobytes() == w.tobytes(), "add(X0); add(X1) against add(X0 ++ X1)"
        for qi in (0, 57, 99):
            alone = a.search(q[qi:qi + 1], k, nprobe)
            for u, v in zip(r1, alone):
                assert u[qi:qi + 1].tobytes() == v.tobytes(), "a query alone against the same query in a batch of 100"
    a.close()
    b.close()


# ---- 7. training ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_training_lowers_the_quantisation_error(pkg, metric):
    m = _metric(pkg, metric)
    rng = np.random.default_rng(9)
    n, d, M, nlist = 10000, 64, 8, 16
    x = _clustered(rng, n, d, 8, 0.7)
    prepared = ref.prepare(int(m), x)
    err = {}
    for niter in (-1, 1, 10):
        ix = pkg.ivfpq_ann.FaissIvfPq.train(m, nlist, M, x, niter=niter, seed=5)
        cb = ix.codebooks()
        assert cb.shape == (M, 256, d // M) and np.all(np.isfinite(cb))
        cent = ix.centroids()
        cells, _ = ref.assign(int(m), prepared, cent)
        # (the training rows' own cells come from the device's assignment; the restatement's agree but for near-ties)
        err[niter] = ref.quantisation_error(ref.residuals(prepared, cent, cells), cb)
        ix.close()
    print("quantisation error per subspace", {k: v.round(5).tolist() for k, v in err.items()})
    assert np.all(err[1] <= err[-1] * (1 + 1e-6))
    assert np.all(err[10] <= err[1] * (1 + 1e-6))


# ---- 8. recall --------------------------------------------------------------------------------------------------------
def test_recall_orderings(pkg):
    m = _metric(pkg, "L2")
    rng = np.random.default_rng(10)
    n, d, nlist, k = 30000, 64, 64, 10
    x = _clustered(rng, n, d, nlist // 4, 1.0)
    dense = pkg.dense_ann.BruteForceIndex.build(m, x)
    q = (x[rng.choice(n, 256)] + rng.standard_normal((256, d))).astype(np.float32)
    t_ids, _, _ = dense.search(q, k)
    dense.close()
    recalls = {}
    for M in (8, 32):
        ix = pkg.ivfpq_ann.FaissIvfPq.train(m, nlist, M, x[:10000], niter=5, seed=2)
        ix.add(x)
        recalls[M] = []
        for nprobe in (1, 8, nlist):
            ids, _, cnt = ix.search(q, k, nprobe)
            recalls[M].append(float(np.mean([len(set(ids[i, :cnt[i]].tolist()) & set(t_ids[i].tolist())) / k for i in range(len(q))])))
        ix.close()
    print("recall@10 at nprobe 1, 8, nlist:", recalls)
    for M in (8, 32):
        assert all(b >= a for a, b in zip(recalls[M], recalls[M][1:])), recalls
    assert recalls[32][-1] >= recalls[8][-1], recalls


# ---- 9. limits --------------------------------------------------------------------------------------------------------
def test_limits_are_refused_and_the_handle_stays_usable(pkg):
    pq = pkg.ivfpq_ann
    m = _metric(pkg, "L2")
    rng = np.random.default_rng(11)
    x = rng.standard_normal((2000, 64)).astype(np.float32)
    for M, what in [(24, "divide"), (6, "multiple of 4"), (128, "4..64")]:
        with pytest.raises(pq.IvfPqError, match=what):
            pq.FaissIvfPq.train(m, 8, M, x)
    with pytest.raises(pq.IvfPqError, match="n_train"):
        pq.FaissIvfPq.train(m, 8, 8, x[:255])
    ix = pq.FaissIvfPq.train(m, 8, 8, x[:256], niter=1)
    ix.add(x)
    before = ix.search(x[:5], 10, 2)
    with pytest.raises(pq.IvfPqError, match="k must"):
        ix.search(x[:5], 1025, 2)
    with pytest.raises(pq.IvfPqError, match="nprobe"):
        ix.search(x[:5], 10, 0)
    with pytest.raises(ValueError, match="codebooks"):
        pq.FaissIvfPq.load(m, ix.centroids(), ix.codebooks()[:, :, :4])
    with pytest.raises(ValueError, match="codebooks"):
        pq.FaissIvfPq.load(m, ix.centroids(), ix.codebooks().reshape(-1))
    after = ix.search(x[:5], 10, 2)
    for u, v in zip(before, after):
        assert u.tobytes() == v.tobytes(), "the handle stays usable"
    ix.search(x[:5], 10, 4096 // 4)
    assert ix.last_probes().shape == (5, 8), "nprobe above nlist is clamped"
    ix.close()


def test_faiss_queryable_and_build_over_the_index(pkg):
    pq, iv = pkg.ivfpq_ann, pkg.ivf_ann
    m = _metric(pkg, "Cosine")
    rng = np.random.default_rng(12)
    x = _clustered(rng, 4000, 64, 8, 0.5)
    ids = np.arange(4000, dtype=np.int64) + 1000
    ix = pq.build_faiss_index(x, ids, 0.5, "IVF16,PQ16x8", m, niter=2)
    assert isinstance(ix, pq.FaissIvfPq) and ix.n == 4000 and ix.M == 16 and ix.nlist == 16
    got = iv.FaissQueryable(ix, m).queryWithDistance(x[17], 5, iv.FaissParams(nprobe=4))
    assert len(got) == 5 and all(0.0 <= dd <= 1.0 for _, dd in got)
    want_ids, want_dist, cnt = ix.search(x[17:18], 5, 4)
    assert [i for i, _ in got] == want_ids[0].tolist()
    flat = pq.build_faiss_index(x, ids, 0.5, "IVF16,Flat", m, niter=2)
    assert isinstance(flat, iv.FaissIvfFlat) and flat.n == 4000
    ix.close()
    flat.close()
