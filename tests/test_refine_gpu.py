"""The re-ranking index on the device (include/refine_ann.h) against the restatement tests/_refine_ref.py, fed with what the
index exports (last_candidates, rows, the base's assignment) -- never with the device's own distances.

Tolerance: the project's 1e-5 / 1e-5 for this arithmetic (fp32 sums of at most 1024 products of fp16 values against float64).
Ids must agree wherever the restatement's neighbours are more than twice that apart; no more than 10 % of the positions of a
test may be left out that way.  The rows are those of tests/test_ivfpq_gpu.py's scan tests (_low_dimensional: 3 latent
dimensions under a random linear map plus 0.3 N(0,1) per component), whose distances spread instead of concentrating:
computed from the restatement alone, without a device, with the k * k_factor NEAREST rows of a query as its candidates (the
densest list a base can hand over), the unclear share over the five (k, k_factor) of a test is at most 0.063 over the 33
queries (Cosine at d = 64; every L2 and InnerProduct case below 0.03) and at most 0.074 for the first query alone (L2 at
d = 200), the worst single (k, k_factor) 0.073.

The bases are loaded from numpy-made centroids and codebooks (a few rows as centroids, residuals of rows as codewords):
training is not the point here."""
import importlib.util
import os

import numpy as np
import pytest

import _refine_ref as ref
from _ivf_ref import low_dimensional as _low_dimensional
from _refine_ref import QUALITY, QUALITY_SEED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ["L2", "Cosine", "InnerProduct"]
MAX_UNCLEAR = 0.10
NLIST, M = 16, 8
# name -> (d of the rows, d the inner index sees, n)
# (opq100: rows of 100 halves, which the store pads to 104; opq200: 25 pieces, fewer than a wave; opq1024: two pieces a lane)
SHAPES = {"pq64": (64, 64, 3000), "pq256": (256, 256, 3000), "opq200": (200, 192, 3000), "opq1024": (1024, 256, 600),
          "opq100": (100, 96, 3000)}
COMBOS = [(1, 1), (10, 1), (10, 8), (100, 10), (256, 4)]  # (k, k_factor); the last is the 1024 boundary


def _metric(pkg, name):
    return getattr(pkg.dense_ann.DistanceMetric, name)


def _numpy_base(metric, y, rng):
    """Centroids and codebooks for rows y as the inner index sees them: NLIST rows, and residuals of 256 rows."""
    import _ivfpq_ref as pq

    rows = ref.prepare(metric, y)
    cent = ref.prepare(metric, y[:NLIST])
    cells, _ = pq.assign(metric, rows, cent)
    res = pq.residuals(rows, cent, cells)
    pick = rng.choice(len(y), 256, replace=False)
    cb = res[pick].reshape(256, M, y.shape[1] // M).transpose(1, 0, 2)
    return y[:NLIST].copy(), np.ascontiguousarray(cb, np.float32)


def _arrays(shape, metric, seed):
    """(x, queries, ids, load arguments of the base) of a shape: everything the index and its twin are built from."""
    d, d_inner, n = SHAPES[shape]
    rng = np.random.default_rng(seed)
    x = _low_dimensional(rng, n + 33, d)
    x, q = x[:n], x[n:]
    ids = rng.permutation(n).astype(np.int64) * 5 + 2
    mi = getattr(ref, {"L2": "L2", "Cosine": "COSINE", "InnerProduct": "INNER_PRODUCT"}[metric])
    if shape.startswith("pq"):
        return x, q, ids, _numpy_base(mi, x, rng)
    A = np.linalg.qr(rng.standard_normal((d, d_inner)))[0].T.astype(np.float32)  # orthonormal rows [d_inner, d]
    xs = x / np.linalg.norm(x, axis=1, keepdims=True) if metric == "Cosine" else x
    cent, cb = _numpy_base(ref.INNER_PRODUCT if metric == "Cosine" else mi, (xs @ A.T).astype(np.float32), rng)
    return x, q, ids, (A, cent, cb)


def _load_base(pkg, shape, metric, args):
    m = _metric(pkg, metric)
    if shape.startswith("pq"):
        return pkg.ivfpq_ann.FaissIvfPq.load(m, *args)
    return pkg.opq_ann.FaissOpqIvfPq.load(m, *args)


_CACHE = {}


@pytest.fixture(scope="module")
def built(pkg):
    def get(shape, metric):
        key = (shape, metric)
        if key not in _CACHE:
            x, q, ids, args = _arrays(shape, metric, 300 + len(shape) + METRICS.index(metric))
            ix = pkg.refine_ann.FaissRefineFlat.wrap(_load_base(pkg, shape, metric, args), k_factor=2)
            ix.add(x, ids)
            _CACHE[key] = (ix, x, q, ids, args, ix.rows().astype(np.float32))
        return _CACHE[key]

    yield get
    for entry in _CACHE.values():
        entry[0].close()
    _CACHE.clear()


def _compare(ix, metric, q, got, k, rows, all_ids, unique_ids=True):
    """got = (ids, dist, cnt) of the last search against the restatement over its exported candidates.  (unclear, total)."""
    got_ids, got_dist, cnt = got
    pos, pc = ix.last_candidates()
    mi = int(ix.metric)
    want = ref.rerank(mi, rows, all_ids, pos, pc, ref.prepare(mi, q), k)
    unclear = total = 0
    for qi, (r_ids, r_dist, _, nxt) in enumerate(want):
        live = pos[qi, :pc[qi]]
        assert len(set(live.tolist())) == len(live) and np.all(live >= 0) and np.all(live < len(rows)), "no position twice"
        assert np.all(pos[qi, pc[qi]:] == -1)
        m = min(k, int(pc[qi]))
        assert cnt[qi] == m, f"query {qi}: count {cnt[qi]} != {m}"
        assert np.all(got_dist[qi, m:] == 0) and np.all(got_ids[qi, m:] == 0), "slots past the count are 0 / 0"
        if m == 0:
            continue
        err = np.abs(got_dist[qi, :m].astype(np.float64) - r_dist)
        tol = ref.ATOL + ref.RTOL * np.abs(r_dist)
        assert np.all(err <= tol), f"query {qi}: error {err.max()} against tolerance {tol[err.argmax()]}"
        assert np.all(np.diff(got_dist[qi, :m]) >= 0), "ascending"
        clear = ref.clear_positions(r_dist, nxt)
        assert np.array_equal(got_ids[qi, :m][clear], r_ids[clear])
        assert not unique_ids or len(set(got_ids[qi, :m].tolist())) == m, "no id twice"
        unclear += int((~clear).sum())
        total += m
    return unclear, total


# ---- 1. the re-rank against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("nq", [1, 33])
def test_rerank_matches_the_restatement(pkg, built, shape, metric, nq):
    ix, x, q, ids, _, rows = built(shape, metric)
    assert ix.n == len(x) and ix.d == SHAPES[shape][0]
    assert np.array_equal(ix.base.assignment()[0], ids)
    assert np.array_equal(rows, ref.prepare(int(ix.metric), x)), "the store holds the rows as ivf_ann.h prepares them"
    unclear = total = 0
    for k, kf in COMBOS:
        got = ix.search(q[:nq], k, 8, kf)
        assert ix.last_candidates()[0].shape == (nq, k * kf)
        u, t = _compare(ix, metric, q[:nq], got, k, rows, ids)
        unclear, total = unclear + u, total + t
        st = ix.last_stats()
        assert st["base_ms"] > 0 and st["rerank_ms"] > 0
    print(f"{shape} {metric} nq={nq}: unclear positions {unclear / total:.4f} of {total}")
    assert unclear <= MAX_UNCLEAR * total, "too many positions unclear: the comparison would be vacuous"


# ---- 2. the candidates are the base's ------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", ["pq64", "opq200"])
def test_candidates_are_what_the_base_answers(pkg, built, shape, metric):
    ix, x, q, ids, args, rows = built(shape, metric)
    twin = _load_base(pkg, shape, metric, args)
    twin.add(x, ids)
    assert np.array_equal(twin.codes(), ix.base.codes())
    for k, kf, nprobe in [(10, 8, 8), (10, 1, 4), (1, 1, 1)]:
        got_ids, got_dist, cnt = ix.search(q, k, nprobe, kf)
        pos, pc = ix.last_candidates()
        b_ids, _, b_cnt = twin.search(q, k * kf, nprobe)
        assert np.array_equal(pc, b_cnt)
        assert np.array_equal(ix.base.last_probes(), twin.last_probes())
        for qi in range(len(q)):
            assert set(ids[pos[qi, :pc[qi]]].tolist()) == set(b_ids[qi, :pc[qi]].tolist())
            assert np.array_equal(ids[pos[qi, :pc[qi]]], b_ids[qi, :pc[qi]]), "and in the base's order"
            if kf == 1:
                assert set(got_ids[qi, :cnt[qi]].tolist()) == set(b_ids[qi, :b_cnt[qi]].tolist()), "k_factor 1 keeps the base's set"
        if kf == 1:  # ... in the order of the true distances
            u, t = _compare(ix, metric, q, (got_ids, got_dist, cnt), k, rows, ids)
            assert u <= MAX_UNCLEAR * max(t, 1) or k == 1
    twin.close()


# ---- 3. short lists and ties -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_short_lists_and_ties(pkg, metric):
    m = _metric(pkg, metric)
    rng = np.random.default_rng(71)
    d = 64
    cent = np.zeros((4, d), np.float32)
    for c in range(4):
        cent[c, c] = 1.0
    cb = (rng.integers(-32, 33, (M, 256, d // M)) / 1024.0).astype(np.float32)
    near0 = (rng.standard_normal((5, d)) * 0.05).astype(np.float16).astype(np.float32)
    near0[:, 0] += 1.0
    one = np.zeros((1, d), np.float32)
    one[0, 1] = 1.0
    ix = pkg.refine_ann.FaissRefineFlat.wrap(pkg.ivfpq_ann.FaissIvfPq.load(m, cent, cb), k_factor=4)
    empty = ix.search(cent, 10, 1)
    assert empty[2].tolist() == [0, 0, 0, 0] and not empty[0].any() and not empty[1].any(), "an empty index answers nothing"
    assert ix.last_candidates()[1].tolist() == [0, 0, 0, 0] and ix.rows().shape == (0, d)
    # cells of 5, 1, 0 and 0 rows; ids: 7 twice on IDENTICAL rows (positions 0 and 5 -> the row of position 0 is added again),
    # and rows 1 and 2 identical under the distinct ids 40 and 30
    x = np.concatenate([near0, one, near0[:1]])
    x[2] = x[1]
    ids = np.array([7, 40, 30, 20, 10, 999, 7], np.int64)
    ix.add(x[:4], ids[:4])
    ix.add(x[4:], ids[4:])
    assert ix.n == 7 and ix.base.list_sizes().tolist() == [6, 1, 0, 0]
    got_ids, got_dist, cnt = ix.search(cent, 10, 1)
    assert cnt.tolist() == [6, 1, 0, 0], "counts of short lists"
    assert np.all(got_ids[2:] == 0) and np.all(got_dist[2:] == 0) and np.all(got_ids[0, 6:] == 0) and np.all(got_dist[0, 6:] == 0)
    assert got_ids[1, 0] == 999
    rows = ix.rows().astype(np.float32)
    _compare(ix, metric, cent, (got_ids, got_dist, cnt), 10, rows, ids, unique_ids=False)
    answer = list(zip(got_dist[0, :6].tolist(), got_ids[0, :6].tolist()))
    assert answer == sorted(answer), "ascending by (distance, id)"
    # the duplicated id: both copies come back, adjacent, with bit-equal distances (equal in distance and id, their order is
    # that of their positions -- which the restatement's positions confirm, the answer itself cannot show it)
    at = np.flatnonzero(got_ids[0, :6] == 7)
    assert len(at) == 2 and at[1] == at[0] + 1 and got_dist[0, at[0]].tobytes() == got_dist[0, at[1]].tobytes()
    want = ref.rerank(int(m), rows, ids, *ix.last_candidates(), ref.prepare(int(m), cent), 10)
    assert want[0][2][at].tolist() == [0, 6]
    # identical rows under distinct ids: id order, bit-equal distances
    a30, a40 = int(np.flatnonzero(got_ids[0, :6] == 30)[0]), int(np.flatnonzero(got_ids[0, :6] == 40)[0])
    assert a40 == a30 + 1 and got_dist[0, a30].tobytes() == got_dist[0, a40].tobytes()
    # k below the count of candidates, k_factor 1: the candidate list is the answer's length
    got_ids, got_dist, cnt = ix.search(cent[:1], 3, 1, 1)
    assert cnt.tolist() == [3] and ix.last_candidates()[0].shape == (1, 3)
    ix.close()


# ---- 4. determinism ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", ["pq64", "opq1024"])
def test_determinism(pkg, built, shape, metric):
    ix, x, q, ids, args, _ = built(shape, metric)
    for k, kf in [(10, 8), (100, 10)]:
        r1 = ix.search(q, k, 8, kf)
        r2 = ix.search(q, k, 8, kf)
        for u, v in zip(r1, r2):
            assert u.tobytes() == v.tobytes(), "search twice"
        alone = ix.search(q[:1], k, 8, kf)
        last = ix.search(np.concatenate([q[1:], q[:1]]), k, 8, kf)
        for u, v, w in zip(r1, alone, last):
            assert u[:1].tobytes() == v.tobytes(), "a query alone against the same query first in a batch of 33"
            assert u[:1].tobytes() == w[-1:].tobytes(), "... and last in it"
    # add(X0); add(X1) against add(X0 ++ X1)
    other = pkg.refine_ann.FaissRefineFlat.wrap(_load_base(pkg, shape, metric, args), k_factor=2)
    cut = len(x) // 3
    other.add(x[:cut], ids[:cut])
    other.add(x[cut:], ids[cut:])
    assert other.rows().tobytes() == ix.rows().tobytes()
    for u, v in zip(ix.search(q, 10, 8, 8), other.search(q, 10, 8, 8)):
        assert u.tobytes() == v.tobytes()
    assert np.array_equal(ix.last_candidates()[0], other.last_candidates()[0])
    other.close()


# ---- 5. failure leaves state ------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_handle_usable(pkg):
    rf = pkg.refine_ann
    x, q, ids, args = _arrays("pq64", "L2", 5)
    base = _load_base(pkg, "pq64", "L2", args)
    ix = rf.FaissRefineFlat.wrap(base, k_factor=4)
    assert ix.k_factor == 4 and ix.base_kind == rf.BASE_IVFPQ and ix.bytes_per_row() == base.bytes_per_row() + 128
    ix.add(x[:1000], ids[:1000])
    before = ix.search(q, 10, 4)
    with pytest.raises(rf.RefineError, match="1025|exceeds"):
        ix.search(q, 205, 4, 5)
    with pytest.raises(rf.RefineError, match="exceeds"):
        ix.search(q, 257, 4)
    with pytest.raises(rf.RefineError, match="k_factor"):
        ix.k_factor = 0
    with pytest.raises(ValueError, match="dimension"):
        ix.add(x[:10, :32], ids[:10])  # (the ABI has no dimension argument: the binding is what can refuse it)
    with pytest.raises(rf.RefineError, match="ids"):
        ix.add(x[1000:1010])  # ids on one add and none on the next
    assert ix.n == 1000 and ix.base.n == 1000 and ix.rows().shape == (1000, 64) and ix.k_factor == 4
    after = ix.search(q, 10, 4)
    for u, v in zip(before, after):
        assert u.tobytes() == v.tobytes(), "the handle stays usable"
    ix.add(x[1000:], ids[1000:])
    assert ix.n == len(x)
    ix.k_factor = 8
    assert ix.k_factor == 8
    for u, v in zip(ix.search(q, 10, 4), ix.search(q, 10, 4, 8)):
        assert u.tobytes() == v.tobytes(), "the index's own factor is the default of a search"
    # a base that holds rows cannot be wrapped, and stays the caller's
    full = _load_base(pkg, "pq64", "L2", args)
    full.add(x[:10])
    with pytest.raises(rf.RefineError, match="holds rows"):
        rf.FaissRefineFlat.wrap(full)
    assert full.n == 10 and full.search(q[:1], 1, NLIST)[2].tolist() == [1]
    full.close()
    ix.close()


# ---- 6. existing behaviour ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ivfpq", "opq"])
def test_plain_searches_answer_as_before_the_position_seam(pkg, kind):
    """ivfpq_search / opq_search on a base that is not wrapped, byte for byte against the answers the library gave before
    ivfpq_internal::search_positions existed (tests/golden/*_search_baseline.npz, written by make_pq_search_baseline.py)."""
    path = os.path.join(ROOT, "tests", "golden", "make_pq_search_baseline.py")
    spec = importlib.util.spec_from_file_location("make_pq_search_baseline", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = np.load(os.path.join(ROOT, "tests", "golden", f"{kind}_search_baseline.npz"))
    got = gen.answers(pkg, kind)
    assert sorted(got) == sorted(want.files) and len(got) == 3 * len(gen.METRICS) * len(gen.SEARCHES)
    for name in sorted(got):
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), name
    assert any(want[n].any() for n in want.files if n.endswith("_dist"))


# ---- 7. quality -------------------------------------------------------------------------------------------------------
def test_refinement_raises_recall(pkg):
    """Clustered low-dimensional corpus (tests/_refine_ref.quality_corpus, seed 7): n = 4000, d = 64, M = 8, nlist = 16,
    nprobe = 16, Cosine, 64 queries; centroids and codebooks by _refine_ref.numpy_train.  Mean recall@10 against the float64
    exhaustive truth.  On the CPU alone (numpy ADC, then _refine_ref.rerank; tests/test_refine_cpu.py asserts it): plain
    ADC 0.2516, k_factor 2 0.4047, k_factor 8 0.8156."""
    m = _metric(pkg, "Cosine")
    p = QUALITY
    x, q = ref.quality_corpus(QUALITY_SEED, p["n"], p["d"], p["nq"])
    cent, cb = ref.numpy_train(ref.COSINE, x, p["nlist"], p["M"], QUALITY_SEED)
    plain = pkg.ivfpq_ann.FaissIvfPq.load(m, cent, cb)
    plain.add(x)
    ix = pkg.refine_ann.FaissRefineFlat.wrap(pkg.ivfpq_ann.FaissIvfPq.load(m, cent, cb), k_factor=8)
    ix.add(x)
    truth = ref.exhaustive(ref.COSINE, ref.prepare(ref.COSINE, x), np.arange(p["n"]), ref.prepare(ref.COSINE, q), p["k"])
    ids, _, cnt = plain.search(q, p["k"], p["nprobe"])
    r_plain = ref.recall(ids, cnt, truth)
    ids, _, cnt = ix.search(q, p["k"], p["nprobe"], 2)
    r2 = ref.recall(ids, cnt, truth)
    ids, dist, cnt = ix.search(q, p["k"], p["nprobe"])
    r8 = ref.recall(ids, cnt, truth)
    print(f"recall@10: plain ivfpq_search {r_plain:.4f}, k_factor 2 {r2:.4f}, k_factor 8 {r8:.4f}; bytes per row "
          f"{plain.bytes_per_row()} -> {ix.bytes_per_row()}; {ix.last_stats()}")
    assert r8 > r_plain, (r_plain, r2, r8)
    assert r8 >= r2, (r_plain, r2, r8)
    # the reference's queryable serves the refined index unchanged
    iv = pkg.ivf_ann
    got = iv.FaissQueryable(ix, m).queryWithDistance(q[3], 5, iv.FaissParams(nprobe=p["nprobe"]))
    assert [i for i, _ in got] == ids[3, :5].tolist() and all(0.0 <= dd <= 1.0 for _, dd in got)
    plain.close()
    ix.close()


def test_build_over_the_factory(pkg):
    rf = pkg.refine_ann
    m = _metric(pkg, "Cosine")
    rng = np.random.default_rng(12)
    x = _low_dimensional(rng, 2000, 72)
    ids = np.arange(2000, dtype=np.int64) + 1000
    ix = rf.build_faiss_index(x, ids, 0.5, "OPQ8_64,IVF16,PQ8,RFlat", m, k_factor=4, niter=2, niter_opq=2)
    assert isinstance(ix, rf.FaissRefineFlat) and ix.base_kind == rf.BASE_OPQ and (ix.n, ix.d, ix.k_factor) == (2000, 72, 4)
    got_ids, got_dist, cnt = ix.search(x[:8], 5, 16, 50)
    assert np.all(cnt == 5) and np.array_equal(got_ids[:, 0], ids[:8]), "a stored row is its own nearest neighbour"
    assert np.all(np.abs(got_dist[:, 0]) <= 1e-3)
    ix.close()
    ix = rf.build_faiss_index(x[:, :64], ids, 0.5, "IVF16,PQ8,Refine(Flat)", m, k_factor=2, niter=2)
    assert ix.base_kind == rf.BASE_IVFPQ and ix.n == 2000
    ix.close()


def test_refined_search_answers_as_before_the_shared_core(pkg):
    """search(q, 10, 4) of a refined ivfpq index (k_factor 4, two adds with ids) and last_candidates(), which pins
    ivfpq_internal::search_positions, byte for byte against what the library gave before ivf_ann.hip and ivfpq_ann.hip
    shared csrc/ivf_core.h (tests/golden/ivf_family_baseline.npz, written by make_ivf_family_baseline.py)."""
    path = os.path.join(ROOT, "tests", "golden", "make_ivf_family_baseline.py")
    spec = importlib.util.spec_from_file_location("make_ivf_family_baseline", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    base = np.load(os.path.join(ROOT, "tests", "golden", "ivf_family_baseline.npz"))
    want = {n: base[n] for n in base.files if n.startswith("refine_")}
    got = gen.refine_answers(pkg)
    assert sorted(got) == sorted(want) and len(got) == 5 * len(gen.METRICS)
    for name in sorted(got):
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), name
    assert any(want[n].any() for n in want if n.endswith("_dist"))


def test_rerank_answers_as_before_the_shared_row_score(pkg):
    """The refine_* blocks of tests/golden/row_score_baseline.npz (written by make_row_score_baseline.py before rerank_kernel
    took its distance, sort and emit from csrc/row_score.h and survivor_topk.h): OPQ bases over rows of 100, 200 and 1024
    components, every metric, (k, k_factor) = (1, 1), (10, 8) and the full sort (256, 4), byte for byte."""
    path = os.path.join(ROOT, "tests", "golden", "make_row_score_baseline.py")
    spec = importlib.util.spec_from_file_location("make_row_score_baseline", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    base = np.load(os.path.join(ROOT, "tests", "golden", "row_score_baseline.npz"))
    want = {n: base[n] for n in base.files if n.startswith("refine_")}
    got, handed = gen.refine_answers(pkg)
    assert sorted(got) == sorted(want) and len(got) == 3 * len(gen.REFINE_DIMS) * len(gen.REFINE_METRICS) * len(gen.SEARCHES)
    for name in sorted(got):
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), name
    assert all(np.all(cnt == 1024) for name, cnt in handed.items() if name.endswith("_256_4"))
    assert all(want[n].any() for n in want if n.endswith("_dist"))
