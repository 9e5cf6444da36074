"""Exhaustive dense search (include/dense_ann.h) on data that is NOT i.i.d. Gaussian: scores that tie in masses, scores
that follow the row position, the best rows in one block -- compared bit for bit, last place included, with a float64
scan.  The contract (above dann_search in the header): with s_k the k-th best fp16-pass score of a query and T the number
of stored rows scoring >= s_k,
  T <= 8192  the search succeeds with the exact top-k, ties in id order, whatever the order / duplication of the rows;
  T >  8192  DANN_ELIMIT (code 3), no answer in the outputs, and the index answers the next search correctly.
T is computed from the reference and each test asserts its side of the contract BEFORE it looks at the device's answer.

Every input has exact arithmetic in fp16 x fp16 -> fp32 (small integers; unit rows with components 1, 1/2, 1/4), so there
is no tolerance anywhere: ids equal in all k places, InnerProduct / Cosine distances bit-equal to float32(1 - dot), L2
distances bit-equal to float32(sqrt(d2)) with d2 the integer squared distance.  (float32(float64 sqrt) of an integer is the correctly rounded
float32 root; the tests require the same bits of the device's sqrtf and allow no ulp on L2 either.)

Kernel constants the shapes are chosen by: 512-row tiles (d <= 256), 8 maxima per tile in pass A, pass A skipped when
8 * full_tiles < k, 8192 survivors per query, 4096 queries per launch."""
import functools
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 8192
L2, COS, IP = 0, 1, 2
METRICS = {"L2": L2, "Cosine": COS, "InnerProduct": IP}


class Ref:
    """Float64 scan of prepared inputs, ordered by np.lexsort((ids, dist)) as oracle.dense_bruteforce orders it; keeps
    the k_max best per query and every sorted distance, from which T(k) follows."""

    def __init__(self, oracle, metric, x, ids, q, k_max):
        px, pq = oracle.dense_prepare(metric, x), oracle.dense_prepare(metric, q)
        assert np.array_equal(px, np.asarray(x, np.float32)) and np.array_equal(pq, np.asarray(q, np.float32)), \
            "the inputs of this file survive the index's preparation unchanged"
        idv = np.arange(len(px), dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
        self.n, m = len(px), min(k_max, len(px))
        self.ids = np.empty((len(pq), m), np.int64)
        self.dist = np.empty((len(pq), m), np.float64)
        self.sorted_dist = np.empty((len(pq), self.n), np.float64)
        for i, row in enumerate(pq):
            dist = oracle.dense_distances(metric, px, row)
            order = np.lexsort((idv, dist))
            self.ids[i], self.dist[i] = idv[order[:m]], dist[order[:m]]
            self.sorted_dist[i] = dist[order]

    def T(self, k):
        """Per query: stored rows at or nearer than the k-th (all of them when k >= n)."""
        kth = self.sorted_dist[:, min(k, self.n) - 1]
        return np.array([np.searchsorted(s, v, side="right") for s, v in zip(self.sorted_dist, kth)])

    def rows(self, sel):
        out = object.__new__(Ref)
        out.n, out.ids, out.dist, out.sorted_dist = self.n, self.ids[sel], self.dist[sel], self.sorted_dist[sel]
        return out


def _assert_exact(res, ref, k):
    ids, dist, cnt = res
    m = min(k, ref.n)
    assert ref.T(k).max() <= CAP, "precondition: the contract promises an answer"
    assert np.array_equal(cnt, np.full(len(cnt), m, np.int32))
    want_d = ref.dist[:, :m].astype(np.float32)
    bad = np.nonzero((ids[:, :m] != ref.ids[:, :m]).any(axis=1))[0]
    assert len(bad) == 0, f"ids differ for queries {bad[:5]} (first at place {np.argmax(ids[bad[0], :m] != ref.ids[bad[0], :m])})"
    assert np.array_equal(dist[:, :m].view(np.int32), want_d.view(np.int32)), "distance bits"


def _assert_refused(pkg, ix, q, k, ref):
    assert ref.T(k).max() > CAP, "precondition: the contract promises a refusal"
    with pytest.raises(pkg.dense_ann.DannError) as e:
        ix.search(q, k)
    assert "error 3" in str(e.value) and "8192" in str(e.value), str(e.value)


def _shuffled_ids(rng, n):
    return rng.permutation(n).astype(np.int64) * 7 + 3


def _metric(pkg, code):
    return pkg.dense_ann.DistanceMetric(code)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _lattice(rng, n, d):
    return rng.integers(-3, 4, size=(n, d)).astype(np.float32)


def _unit_rows(rng, n, d):
    """Rows of exactly unit norm with fp16-exact components: signed one-hot, four of +-1/2, sixteen of +-1/4."""
    x = np.zeros((n, d), np.float32)
    for i in range(n):
        cnt, val = ((1, 1.0), (4, 0.5), (16, 0.25))[i % 3]
        at = rng.choice(d, size=cnt, replace=False)
        x[i, at] = val * rng.choice([-1.0, 1.0], size=cnt)
    return x


@functools.lru_cache(maxsize=None)
def _case1(metric, with_ids):
    rng = np.random.default_rng(1)
    make = _unit_rows if metric == COS else _lattice
    x, q = make(rng, 30000, 32), make(rng, 33, 32)
    ids = _shuffled_ids(rng, len(x)) if with_ids else None
    return x, q, ids


@functools.lru_cache(maxsize=None)
def _case1_ref(oracle, metric, with_ids):
    x, q, ids = _case1(metric, with_ids)
    return Ref(oracle, metric, x, ids, q, 1024)


def _near_origin(rng, count):
    """`count` distinct integer rows (dims 1..4) with 0 < |x|^2 < 16."""
    pts = [p for p in itertools.product(range(-3, 4), repeat=4) if 0 < sum(c * c for c in p) < 16]
    return np.array(pts, np.float32)[rng.permutation(len(pts))[:count]]


def _tie_mass(metric, B, place, n=40000, d=32, seed=5, zero_mass=False):
    """n rows of which n - B share one score (the mass) and B score strictly better, for the query returned.
    InnerProduct: every row is e0, the B also carry 1..B in component 1, q = e0 + 2 e1 (mass 1, better 1 + 2j).
    L2: copies of 4 e0 and B distinct integer rows with |x| < 4, q = 0.
    zero_mass (InnerProduct): the mass is all-zero rows, the B are j e1, q = e1 (mass 0, better j)."""
    rng = np.random.default_rng(seed + B)
    if place == "last" and B > 64:
        n = n - n % 512 + 256  # 40000 leaves 64 rows in the partial tile: make it 256, so that all B lie inside it
    if place == "scattered":
        at = rng.choice(n, size=B, replace=False)
    elif place == "first":  # inside the first tile
        at = rng.choice(512, size=B, replace=False)
    else:  # the last B rows: all inside the partial last tile
        assert B <= n % 512
        at = np.arange(n - B, n)
    x = np.zeros((n, d), np.float32)
    q = np.zeros((1, d), np.float32)
    if zero_mass:
        x[at, 1] = rng.permutation(B).astype(np.float32) + 1.0
        q[0, 1] = 1.0
    elif metric == IP:
        x[:, 0] = 1.0
        x[at, 1] = rng.permutation(B).astype(np.float32) + 1.0
        q[0, 0], q[0, 1] = 1.0, 2.0
    else:
        x[:, 0] = 4.0
        x[at] = 0.0
        x[at, 1:5] = _near_origin(rng, B)
    return x, q


# ---- 1: natural ties at every boundary ---------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("with_ids", [False, True], ids=["positions", "shuffled_ids"])
@pytest.mark.parametrize("metric", ["L2", "Cosine", "InnerProduct"])
def test_natural_ties_at_every_boundary(pkg, oracle, metric, with_ids, exact):
    """Lattice rows (Cosine: unit rows of three shapes), n = 30000, d = 32, 33 queries, k in {1, 10, 100, 1024}: most
    k-th places fall inside a group of equal scores, so the id-ascending rule decides the cut.  k = 1024 has too few tiles
    for pass A (58 full tiles x 8 < 1024) and goes through the overflow refinement.  In exact mode fp32 equals fp16 on
    this data, so the same answer is required."""
    m = METRICS[metric]
    x, q, ids = _case1(m, with_ids)
    ref = _case1_ref(oracle, m, with_ids)
    ix = pkg.dense_ann.BruteForceIndex.build(_metric(pkg, m), x, ids, exact=exact)
    try:
        for k in (1, 10, 100, 1024):
            _assert_exact(ix.search(q, k), ref, k)
    finally:
        ix.close()


# ---- 2: a tie mass below the k-th --------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", ["scattered", "first", "last"])
@pytest.mark.parametrize("k", [4, 10, 100])
@pytest.mark.parametrize("extra", ["k", "k+2", "2k"])
@pytest.mark.parametrize("metric", ["InnerProduct", "L2"])
def test_tie_mass_below_the_kth_is_not_a_limit(pkg, oracle, metric, extra, k, place):
    """40000 - B rows (40192 - B where the partial last tile has to hold more than 64 better rows) tie at one score and
    B >= k rows beat it: T <= B, the answer is the k best of the B.  Pass A's
    sample sees few of the B, tau lands on the mass, the buffer overflows with an arbitrary 8192 of the 40000 -- and the
    search must still get above the mass instead of reporting a tie at the k-th that does not exist."""
    m = METRICS[metric]
    B = {"k": k, "k+2": k + 2, "2k": 2 * k}[extra]
    x, q = _tie_mass(m, B, place)
    ref = Ref(oracle, m, x, None, q, k)
    assert ref.T(k).max() <= B
    ix = pkg.dense_ann.BruteForceIndex.build(_metric(pkg, m), x)
    try:
        got = ix.search(q, k)
        print(f"tie mass {metric} B={B} k={k} {place}: {ix.last_rounds()} rounds")
        _assert_exact(got, ref, k)
    finally:
        ix.close()


@pytest.mark.parametrize("metric", ["InnerProduct", "L2"])
def test_tie_mass_of_8193_rows(pkg, oracle, metric):
    """The smallest mass that overflows the buffer: 8193 tied rows and B = 20 better ones, k = 10."""
    m = METRICS[metric]
    x, q = _tie_mass(m, 20, "scattered", n=8193 + 20)
    ref = Ref(oracle, m, x, None, q, 10)
    ix = pkg.dense_ann.BruteForceIndex.build(_metric(pkg, m), x)
    try:
        _assert_exact(ix.search(q, 10), ref, 10)
    finally:
        ix.close()


@pytest.mark.parametrize("place", ["scattered", "last"])
def test_tie_mass_of_all_zero_rows(pkg, oracle, place):
    """Cold-start rows: the mass is all-zero rows scoring 0 under InnerProduct, B = 20 rows score 1..20, k = 10.  The float
    above the mass's score is then the smallest subnormal, which the threshold test has to honour."""
    x, q = _tie_mass(IP, 20, place, zero_mass=True)
    ref = Ref(oracle, IP, x, None, q, 10)
    assert ref.T(10)[0] == 10
    ix = pkg.dense_ann.BruteForceIndex.build(_metric(pkg, IP), x)
    try:
        got = ix.search(q, 10)
        print(f"all-zero mass, {place}: {ix.last_rounds()} rounds")
        _assert_exact(got, ref, 10)
    finally:
        ix.close()


# ---- 3: true refusal, and recovery -------------------------------------------------------------------------------------
def test_true_refusal_then_recovery(pkg, oracle):
    """B = 20 better rows and k = 21: the 21st best IS the mass, T = 40000 -- refused, with the limit in the message; the
    same handle then answers k = 10 exactly."""
    x, q = _tie_mass(IP, 20, "scattered")
    ref = Ref(oracle, IP, x, None, q, 21)
    assert ref.T(21)[0] == 40000 and ref.T(10)[0] == 10
    ix = pkg.dense_ann.BruteForceIndex.build(_metric(pkg, IP), x)
    try:
        _assert_refused(pkg, ix, q, 21, ref)
        _assert_exact(ix.search(q, 10), ref, 10)
        _assert_refused(pkg, ix, q, 21, ref)
        _assert_exact(ix.search(q, 20), ref, 20)
    finally:
        ix.close()


@pytest.mark.parametrize("n", [8192, 8193])
def test_identical_rows_at_the_buffer_size(pkg, oracle, n):
    """n identical rows, k = 100: T = n.  8192 fit the buffer -- the 100 smallest ids at equal distances; 8193 do not."""
    rng = np.random.default_rng(n)
    x = np.zeros((n, 16), np.float32)
    x[:, 0], x[:, 3] = 1.0, -2.0
    q = x[:1].copy()
    ids = _shuffled_ids(rng, n)
    ref = Ref(oracle, IP, x, ids, q, 100)
    assert ref.T(100)[0] == n
    ix = pkg.dense_ann.BruteForceIndex.build(_metric(pkg, IP), x, ids)
    try:
        if n <= CAP:
            got = ix.search(q, 100)
            _assert_exact(got, ref, 100)
            assert np.array_equal(got[0][0], np.sort(ids)[:100]) and len(set(got[1][0].tolist())) == 1
        else:
            _assert_refused(pkg, ix, q, 100, ref)
    finally:
        ix.close()


def test_one_refusable_query_fails_the_call_and_nothing_else(pkg, oracle):
    """A batch with one query beyond the limit fails as a whole (the documented behaviour), writes no count a caller could
    take for an answer, and the same batch without that query is exact on the same handle."""
    x, _ = _tie_mass(IP, 20, "scattered")
    q = np.zeros((9, 32), np.float32)
    q[:, 0] = 1.0
    q[:, 1] = [1, 2, 3, 4, 0, 5, 6, 7, 8]  # row 4 is e0: all 40000 rows score 1
    ref = Ref(oracle, IP, x, None, q, 10)
    T = ref.T(10)
    assert T[4] == 40000 and np.delete(T, 4).max() <= CAP
    ix = pkg.dense_ann.BruteForceIndex.build(_metric(pkg, IP), x)
    try:
        lib = pkg.dense_ann._lib()
        dist = np.full((9, 10), -7.0, np.float32)
        ids = np.full((9, 10), -7, np.int64)
        cnt = np.full(9, -7, np.int32)
        rc = lib.dann_search(ix._h, 9, q.ctypes.data, 10, dist.ctypes.data, ids.ctypes.data, cnt.ctypes.data)
        assert rc == 3 and b"8192" in lib.dann_last_error()
        assert np.all(cnt == 0), "a failed search reports no neighbours for any query"
        with pytest.raises(pkg.dense_ann.DannError):
            ix.search(q, 10)
        keep = np.array([0, 1, 2, 3, 5, 6, 7, 8])
        _assert_exact(ix.search(q[keep], 10), ref.rows(keep), 10)
    finally:
        ix.close()


# ---- 4: score correlated with position ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ordered(descending):
    n = 40000
    i = np.arange(n)
    if descending:
        i = i[::-1]
    x = np.zeros((n, 16), np.float32)
    x[:, 0], x[:, 1] = i // 256, i % 256
    q = np.zeros((1, 16), np.float32)
    q[0, 0], q[0, 1] = 256.0, 1.0  # score of the row holding i is exactly i
    return x, q


@pytest.mark.parametrize("k", [10, 1024])
@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
def test_score_follows_position(pkg, oracle, descending, k):
    """x_i = (i // 256, i % 256, 0, ...), q = (256, 1, 0, ...): the score is the row number (or its mirror).  k = 1024
    has no pass A at n = 40000, every row is emitted, and refinement starts from whichever 8192 arrived first -- with the
    workgroups running in position order that is one end of the score range, never a fair sample.  k = 10 takes the
    sampled pass."""
    x, q = _ordered(descending)
    ref = Ref(oracle, IP, x, None, q, k)
    assert ref.T(k)[0] == k
    ix = pkg.dense_ann.BruteForceIndex.build(_metric(pkg, IP), x)
    try:
        got = ix.search(q, k)
        rounds = ix.last_rounds()
        print(f"ordered scores, descending={descending}, k={k}: {rounds} rounds")
        _assert_exact(got, ref, k)
        best = np.arange(39999, 39999 - k, -1)
        assert np.array_equal(got[0][0], 39999 - best if descending else best)
        if k == 1024:
            assert rounds >= 2, "40000 emitted rows cannot fit 8192 slots: a second pass is certain"
    finally:
        ix.close()


# ---- 5: the best rows in one contiguous block --------------------------------------------------------------------------
@pytest.mark.parametrize("k", [100, 1024])
def test_best_rows_in_one_block_built_or_appended(pkg, oracle, k):
    """Lattice rows, n = 30000, d = 64, rows 12000..16999 moved by +4 u, queries around 2 u: every neighbour lies in one
    run of ten tiles.  Built in one call, and built from rows 0..11999 with the rest appended in two calls under shuffled
    ids, so that selection orders ties by the id rank (rank / rpos): both equal the reference, hence each other."""
    rng = np.random.default_rng(11)
    n, d = 30000, 64
    x = _lattice(rng, n, d)
    u = rng.integers(-1, 2, size=d).astype(np.float32)
    x[12000:17000] += 4.0 * u
    q = 2.0 * u[None, :] + rng.integers(-1, 2, size=(8, d)).astype(np.float32)
    ids = _shuffled_ids(rng, n)
    ref = Ref(oracle, IP, x, ids, q, k)
    at = np.argsort(ids)[np.searchsorted(np.sort(ids), ref.ids)]  # positions of the reference's neighbours
    assert at.min() >= 12000 and at.max() < 17000
    B = pkg.dense_ann.BruteForceIndex
    one = B.build(_metric(pkg, IP), x, ids)
    grown = B.build(_metric(pkg, IP), x[:12000], ids[:12000])
    try:
        grown.append(x[12000:21000], ids[12000:21000])
        grown.append(x[21000:], ids[21000:])
        a, b = one.search(q, k), grown.search(q, k)
        _assert_exact(a, ref, k)
        _assert_exact(b, ref, k)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    finally:
        one.close()
        grown.close()


# ---- 6: the 4096-query chunk boundary of dann_search -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chunk_case(oracle, metric):
    rng = np.random.default_rng(6)
    x, q = _lattice(rng, 600, 16), _lattice(rng, 4097, 16)
    return x, q, Ref(oracle, metric, x, None, q, 5)


@pytest.mark.parametrize("nq", [4096, 4097])
@pytest.mark.parametrize("metric", ["InnerProduct", "L2"])
def test_query_chunk_boundary(pkg, oracle, metric, nq):
    """One launch holds 4096 queries; the 4097th opens a second chunk of one query (n = 600, d = 16, k = 5)."""
    m = METRICS[metric]
    x, q, ref = _chunk_case(oracle, m)
    ix = pkg.dense_ann.BruteForceIndex.build(_metric(pkg, m), x)
    try:
        _assert_exact(ix.search(q[:nq], 5), ref.rows(slice(0, nq)), 5)
    finally:
        ix.close()


# ---- 7: exact mode on the tie mass -------------------------------------------------------------------------------------
def test_exact_mode_on_the_tie_mass(pkg, oracle):
    """The tie mass (InnerProduct, B = 2k, k = 10) in exact mode, where tau starts below the pass-A bound by the rounding
    slack and so may lie inside or under the mass: the exact answer or DANN_ELIMIT, never a wrong answer, and the handle
    stays usable (three searches in a row, each held to the same rule).  On an MI355X: the exact answer in 3 passes for
    each (dense exhaustive search); the kernel before the probe refused all three."""
    x, q = _tie_mass(IP, 20, "scattered")
    q2 = q.copy()
    q2[0, 1] = 3.0
    ix = pkg.dense_ann.BruteForceIndex.build(_metric(pkg, IP), x, exact=True)
    try:
        for query in (q, q2, q):
            ref = Ref(oracle, IP, x, None, query, 10)
            assert ref.T(10)[0] == 10
            try:
                got = ix.search(query, 10)
            except pkg.dense_ann.DannError as e:
                print("exact mode on the tie mass: refused:", e)
                assert "error 3" in str(e)
                continue
            print("exact mode on the tie mass: answered in", ix.last_rounds(), "rounds")
            _assert_exact(got, ref, 10)
    finally:
        ix.close()
