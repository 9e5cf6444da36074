"""The Annoy index on the device (include/annoy_ann.h) against the restatement tests/_annoy_ref.py, fed with what the index
exports (its forest, its stored rows) and the prepared queries -- never with the device's own margins or distances.

Candidates and pops must agree exactly: the walk is integer-exact once the float32 margins are (they are stated to the bit).
Answers: the project's 1e-5 / 1e-5 against the float64 re-score of the restatement's candidates; ids must agree wherever the
restatement's neighbours are more than twice that apart, and no more than 10 % of a test's positions may be left out that
way.  The rows are test_refine_gpu.py's _low_dimensional (3 latent dimensions under a random linear map plus 0.3 N(0,1) per
component), n = 3000 with 33 queries.  Computed from the restatement alone, without a device (forest and preparation are
host code), the unclear share of each case of CASES, in order: 0.000, 0.070, 0.027, 0.025, 0.071, 0.021, 0.036, 0.000,
0.006, 0.042, 0.025; the exhaustive test: 0.000 (L2), 0.027 (Cosine); the hand-made forest: at most 0.006 (L2) and 0.030
(Cosine, where the all-zero query ties every row at distance 1) over its five budgets.

CASES covers d in {3, 64, 100, 200, 1024} (one partial piece; padding to 104; 25 pieces, fewer than a wave; two pieces a
lane), both metrics, 1, 7 and 80 trees, leaf sizes 2 and d + 2, k in {1, 10, 200, 1024} and nodes_to_explore none, 0, below
n_trees * k and 20000; cases 5 and 6 hand the selection more than 1024 candidates (the radix passes)."""
import functools

import numpy as np
import pytest

import _annoy_ref as ref
from _pkg import load_package

pytestmark = pytest.mark.gpu

L2, COSINE = ref.L2, ref.COSINE
N, NQ = 3000, 33
MAX_UNCLEAR = 0.10
# (d, metric, n_trees, leaf_size, k, nodes_to_explore, caller ids)
CASES = [(3, L2, 1, 2, 1, None, False), (3, COSINE, 7, 0, 10, 0, True), (64, COSINE, 80, 0, 10, 20000, False),
         (64, L2, 7, 2, 200, 100, True), (100, L2, 7, 0, 1024, None, False), (100, COSINE, 1, 2, 10, 20000, True),
         (200, COSINE, 7, 0, 10, 20000, False), (200, L2, 80, 0, 1, None, True), (1024, L2, 7, 0, 10, 0, False),
         (1024, COSINE, 1, 2, 200, None, True), (64, L2, 80, 0, 200, None, False)]


def _an():
    return load_package().annoy_ann


@functools.lru_cache(maxsize=None)
def _data(d, n=N, seed=5):
    """(rows, queries, caller ids)"""
    rng = np.random.default_rng(seed + d)
    x = ref.low_dimensional(rng, n + NQ, d)
    return x[:n], x[n:], rng.permutation(n).astype(np.int64) * 5 + 2


@functools.lru_cache(maxsize=None)
def _forest(d, metric, n_trees, leaf_size):
    """(library forest, its arrays, prepared rows, prepared queries): host code only."""
    an = _an()
    x, q, _ = _data(d)
    f = an.AnnoyForest.build(metric, x, n_trees, leaf_size, seed=3)
    return f, ref.forest_arrays(f), an.prepare(metric, x).astype(np.float32), an.prepare(metric, q).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(case):
    """The restatement's (candidates, pops, collected, re-scored answers) of a case: no device."""
    d, metric, n_trees, leaf_size, k, nte, own_ids = case
    _, fa, rows, qp = _forest(d, metric, n_trees, leaf_size)
    ids = _data(d)[2] if own_ids else np.arange(1, N + 1)
    cands, pops, coll = ref.walk_all(fa, qp, ref.search_k(n_trees, k, nte))
    return cands, pops, coll, ref.rescore(metric, rows, ids, cands, qp, k)


def _index(d, metric, n_trees, leaf_size, own_ids=False):
    f = _forest(d, metric, n_trees, leaf_size)[0]
    x, _, ids = _data(d)
    return _an().AnnoyQueryable.from_forest(f, x, ids if own_ids else None)


def _same_candidates(ix, cands):
    pos, cnt = ix.last_candidates()
    assert cnt.tolist() == [len(c) for c in cands]
    for q, c in enumerate(cands):
        assert np.array_equal(pos[q, :cnt[q]], c), q
        assert np.all(pos[q, cnt[q]:] == -1)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "d%d-m%d-t%d-l%d-k%d-e%s-i%d" % c)
def test_candidates_and_answers_follow_the_restatement(case):
    d, metric, n_trees, leaf_size, k, nte, own_ids = case
    cands, pops, coll, res = _reference(case)
    assert ref.unclear_share(res) <= MAX_UNCLEAR  # a condition on the case, from the restatement alone
    ix = _index(d, metric, n_trees, leaf_size, own_ids)
    fa, rows = _forest(d, metric, n_trees, leaf_size)[1:3]
    assert np.array_equal(ix.rows().astype(np.float32), rows)
    assert all(np.array_equal(a, b) for a, b in zip(ref.forest_arrays(ix.forest()).values(), fa.values()))
    ids, dist, cnt = ix.search(_data(d)[1], k, nte)
    _same_candidates(ix, cands)
    st = ix.last_stats()
    assert np.array_equal(st["pops"], pops) and np.array_equal(st["collected"], coll)
    assert st["slices"] == 1 and st["rerun"] == 0
    clear, total = ref.check_answers(res, ids, dist, cnt, k)
    assert total - clear <= MAX_UNCLEAR * total
    ix.close()


@pytest.mark.parametrize("metric", [L2, COSINE])
def test_exhaustive_budget_answers_the_exhaustive_search(metric):
    """search_k = n_trees * n reaches every leaf: the answer is the float64 exhaustive one (no walk of the restatement)."""
    d, n_trees, k = 64, 7, 10
    _, _, rows, qp = _forest(d, metric, n_trees, 0)
    ix = _index(d, metric, n_trees, 0)
    ids, dist, cnt = ix.search(_data(d)[1], k, n_trees * N)
    pos, ccnt = ix.last_candidates()
    assert np.all(ccnt == N) and np.array_equal(pos, np.tile(np.arange(N, dtype=np.int32), (NQ, 1)))
    res = ref.exhaustive(metric, rows, np.arange(1, N + 1), qp, k)
    clear, total = ref.check_answers(res, ids, dist, cnt, k)
    assert total == NQ * k and total - clear <= MAX_UNCLEAR * total
    ix.close()


@pytest.mark.parametrize("leaf_size", [2, 0])
@pytest.mark.parametrize("metric", [L2, COSINE])
def test_stored_rows_find_themselves(metric, leaf_size):
    d = 100
    ix = _index(d, metric, 1, leaf_size)
    x = _data(d)[0]
    ids, dist, cnt = ix.search(x[:256], 1, None)
    assert np.all(cnt == 1) and np.array_equal(ids[:, 0], np.arange(1, 257))
    if metric == L2:
        assert not dist.any()  # exactly 0
    else:  # 1 - |row|^2 of the row as stored: its halves are a unit vector only up to their rounding
        rows = _forest(d, metric, 1, leaf_size)[2][:256].astype(np.float64)
        assert np.allclose(dist[:, 0], 1.0 - (rows * rows).sum(axis=1), rtol=ref.RTOL, atol=ref.ATOL)
    ix.close()


def test_batches_repeats_and_k_above_n():
    d, metric, k = 64, COSINE, 10
    ix = _index(d, metric, 7, 0, own_ids=True)
    q = _data(d)[1]
    base = ix.search(q, k, 2000)
    again = ix.search(q, k, 2000)
    assert all(np.array_equal(a, b) for a, b in zip(base, again))
    for width in (65, 4097):
        big = np.tile(q, (width // NQ + 1, 1))[:width]
        got = ix.search(big, k, 2000)
        for i in (0, 1, 32, 33, 64, width - 1):
            for a, b in zip(got, base):
                assert a[i].tobytes() == b[i % NQ].tobytes()
    for i in (0, 17):
        one = ix.search(q[i:i + 1], k, 2000)
        for a, b in zip(one, base):
            assert a[0].tobytes() == b[i].tobytes()
    # search_k = 7 * 40000 is above the limit: refused, and the index serves on
    with pytest.raises(_an().AnnoyError, match="error 3: search_k = 280000 exceeds 262144"):
        ix.search(q, k, 7 * 40000)
    assert all(np.array_equal(a, b) for a, b in zip(ix.search(q, k, 2000), base))
    ix.close()
    # k above n: every row, then 0 / 0
    an = _an()
    x = _data(d)[0][:50]
    small = an.AnnoyQueryable.build(L2, x, 1, leaf_size=4)
    ids, dist, cnt = small.search(q[:5], 200)
    assert np.all(cnt == 50) and not ids[:, 50:].any() and not dist[:, 50:].any()
    assert all(sorted(ids[i, :50].tolist()) == list(range(1, 51)) for i in range(5))
    assert np.all(np.diff(dist[:, :50], axis=1) >= 0)
    small.close()


def test_queue_overflow_is_rerun_with_room_for_every_node():
    d, metric, n_trees, k = 64, L2, 7, 10
    ix = _index(d, metric, n_trees, 2)
    q = _data(d)[1]
    base = ix.search(q, k, 5000)
    base_cands = ix.last_candidates()
    assert ix.last_stats()["rerun"] == 0
    ix.debug_set_limits(first_queue_capacity=n_trees + 8)
    got = ix.search(q, k, 5000)
    st = ix.last_stats()
    assert st["rerun"] == NQ  # (a walk of thousands of pops outgrows 15 entries for every query)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, base))
    assert all(np.array_equal(a, b) for a, b in zip(ix.last_candidates(), base_cands))
    # a scratch budget below one full-size queue: the re-run goes one query at a time
    ix.debug_set_limits(first_queue_capacity=n_trees + 8, scratch_budget_bytes=1)
    got = ix.search(q, k, 5000)
    assert ix.last_stats()["rerun"] == NQ and ix.last_stats()["slices"] == NQ
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, base))
    ix.debug_set_limits()
    ix.close()


def test_slices_give_the_same_bytes():
    """A scratch budget of 67 queries' worth cuts a batch of 200 into three slices.  Per query the scratch is the queue
    (8 bytes an entry), the set (4 bytes a slot, a power of two at least twice the candidates) and the keys (8 bytes a
    candidate); the candidate lists of a batch this small stay outside the budget, for the export."""
    d, metric, n_trees, k, nte = 64, COSINE, 7, 10, 2000
    ix = _index(d, metric, n_trees, 0)
    fa = _forest(d, metric, n_trees, 0)[1]
    q = np.tile(_data(d)[1], (7, 1))[:200]
    base = ix.search(q, k, nte)
    assert ix.last_stats()["slices"] == 1
    max_leaf = int(fa["nodes"][fa["nodes"][:, 0] == ref.LEAF][:, 2].max())
    cand_cap = min(N, ref.search_k(n_trees, k, nte) - 1 + max_leaf)
    table_cap = 64
    while table_cap < 2 * cand_cap:
        table_cap *= 2
    heap_cap = min(len(fa["nodes"]), n_trees + 16384)
    ix.debug_set_limits(scratch_budget_bytes=67 * (heap_cap * 8 + table_cap * 4 + cand_cap * 8))
    got = ix.search(q, k, nte)
    assert ix.last_stats()["slices"] == 3
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, base))
    pos, cnt = ix.last_candidates()
    assert np.array_equal(pos[:NQ], pos[165:198]) and np.array_equal(cnt[:NQ], cnt[165:198])
    ix.close()


def _hand_made(d=8, n=64):
    """Tree 0: a chain (every split's left child a leaf of 2, its right child the next split; the last holds two leaves).
    Tree 1: a root with a ZERO normal over two leaves of 32: both children tie at bound 0 and the node number decides."""
    rng = np.random.default_rng(12)
    nodes, normals, offsets = [], [], []
    links = n // 2 - 1
    for i in range(links):  # split 2i, its left leaf 2i + 1
        last = i == links - 1
        nodes.append([ref.SPLIT, 2 * i + 1, 2 * i + 2, 0])
        nodes.append([ref.LEAF, 2 * i, 2, 0])
        if last:
            nodes.append([ref.LEAF, 2 * i + 2, 2, 0])
        normals.append(rng.standard_normal(d))
        offsets.append(rng.standard_normal() * 0.1)
    root1 = len(nodes)
    nodes += [[ref.SPLIT, root1 + 1, root1 + 2, 0], [ref.LEAF, n, 32, 0], [ref.LEAF, n + 32, 32, 0]]
    normals.append(np.zeros(d))
    offsets.append(0.0)
    items = np.concatenate([rng.permutation(n), rng.permutation(n)]).astype(np.int32)
    return dict(d=d, n=n, leaf_size=32, nodes=np.array(nodes, np.int32), normals=np.array(normals, np.float16),
                offsets=np.array(offsets, np.float32), roots=np.array([0, root1], np.int32), items=items)


@pytest.mark.parametrize("metric", [L2, COSINE])
def test_hand_made_forest_is_walked_as_the_restatement_walks_it(metric):
    an = _an()
    fa = dict(_hand_made(), metric=metric)
    if metric == COSINE:
        fa["offsets"] = np.zeros_like(fa["offsets"])
    rng = np.random.default_rng(4)
    x = rng.standard_normal((fa["n"] + NQ, fa["d"])).astype(np.float32)
    x, q = x[:fa["n"]], x[fa["n"]:]
    q[0] = 0  # every margin of the chain is its offset (L2) or 0 (Cosine)
    f = an.AnnoyForest.load(**fa)
    ix = an.AnnoyQueryable.from_forest(f, x)
    rows, qp = an.prepare(metric, x).astype(np.float32), an.prepare(metric, q).astype(np.float32)
    for k, nte in ((1, None), (1, 8), (3, 40), (10, 66), (64, None)):
        cands, pops, coll = ref.walk_all(fa, qp, ref.search_k(2, k, nte))
        ids, dist, cnt = ix.search(q, k, nte)
        _same_candidates(ix, cands)
        st = ix.last_stats()
        assert np.array_equal(st["pops"], pops) and np.array_equal(st["collected"], coll)
        res = ref.rescore(metric, rows, np.arange(1, fa["n"] + 1), cands, qp, k)
        clear, total = ref.check_answers(res, ids, dist, cnt, k)
        assert total - clear <= MAX_UNCLEAR * total
    ix.close()


@pytest.mark.parametrize("metric", [L2, COSINE])
def test_duplicates_come_in_id_order(metric):
    d, n_trees = 64, 7
    an = _an()
    x, q, ids = (a.copy() for a in _data(d))
    rng = np.random.default_rng(8)
    dup = rng.choice(N, 40, replace=False)
    x[dup] = q[0]
    ix = an.AnnoyQueryable.build(metric, x, n_trees, ids, seed=2)
    got_ids, got_dist, cnt = ix.search(q[:1], 64, n_trees * N)
    assert cnt[0] == 64
    assert got_ids[0, :40].tolist() == sorted(ids[dup].tolist())
    assert np.all(got_dist[0, :40] == got_dist[0, 0]) and got_dist[0, 40] > got_dist[0, 0]
    if metric == L2:
        assert got_dist[0, 0] == 0
    order = np.lexsort((got_ids[0, :64], got_dist[0, :64]))
    assert np.array_equal(order, np.arange(64))
    ix.close()


def test_quality():
    """recall@10 against the float64 exhaustive search on _annoy_ref.quality_data() (n = 4000, d = 64, 64 queries, Cosine, 20
    trees, no nodesToExplore).  An equally valid builder sets the bar: _annoy_ref.numpy_forest over seeds 0..7, searched by
    the restatement, measured on the CPU: 0.9516, 0.9641, 0.9719, 0.9812, 0.9703, 0.9703, 0.9750, 0.9750 (worst 0.9516,
    standard deviation 0.0083); the library's forest searched by the restatement: 0.9609.  The library must not fall below
    the worst of the eight minus their standard deviation: a split that is balanced but useless would."""
    numpy_recalls = np.array([0.9516, 0.9641, 0.9719, 0.9812, 0.9703, 0.9703, 0.9750, 0.9750])
    bar = numpy_recalls.min() - numpy_recalls.std()
    an = _an()
    p = ref.QUALITY
    x, q = ref.quality_data()
    ix = an.AnnoyQueryable.build(COSINE, x, p["n_trees"], seed=1)
    ids, _, cnt = ix.search(q, p["k"])
    rows, qp = an.prepare(COSINE, x).astype(np.float32), an.prepare(COSINE, q).astype(np.float32)
    truth = ref.exhaustive(COSINE, rows, np.arange(1, p["n"] + 1), qp, p["k"])
    got = ref.recall(ids, cnt, truth)
    print(f"recall@10 {got:.4f}, bar {bar:.4f}")
    assert got >= bar
    ix.close()


def test_answers_as_before_the_shared_row_score():
    """The annoy_* blocks of tests/golden/row_score_baseline.npz (written by make_row_score_baseline.py before walk_kernel,
    score_kernel and select_kernel took their loads, distance and emit from csrc/row_score.h): d in {3, 100, 200, 1024}, both
    metrics, k = 10, and one search that hands the selection more than 1024 candidates; answers, pops and collected byte
    for byte.  The digests of the forest and of the stored rows are host code: they are compared first, so that a host-side
    difference is not taken for a kernel's."""
    import importlib.util
    import os

    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_row_score_baseline", os.path.join(golden, "make_row_score_baseline.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    base = np.load(os.path.join(golden, "row_score_baseline.npz"))
    want = {n: base[n] for n in base.files if n.startswith("annoy_")}
    got, handed = gen.annoy_answers(load_package())
    assert sorted(got) == sorted(want) and len(got) == (2 + 5) * len(gen.ANNOY_DIMS) * len(gen.ANNOY_METRICS) + 5
    for name in sorted(got, key=lambda n: (not n.endswith("_sha256"), n)):
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), name
    assert np.all(handed["annoy_%d_%s_%d_%d" % gen.ANNOY_WIDE[:4]] > 1024)
    assert all(want[n].any() for n in want if n.endswith("_dist"))
