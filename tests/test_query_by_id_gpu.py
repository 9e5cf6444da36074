"""Query by id from a device embedding store (include/ann_by_id.h) against the host composition it replaces: for each seed in
order, if the store holds it, index.search(store_rows[seed][None], k[, ef]), flattened on the host.  Both sides run the same
preparation arithmetic on the same fp32 rows and the same search kernels, so everything is compared bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_INDEX, N_STORE, N_SEEDS = 20000, 50000, 4096
STORE_KEY0 = 1_000_000_000  # user ids; the index's ids (tweets) are 5 + 7 i: disjoint


def _metrics(pkg):
    m = pkg.dense_ann.DistanceMetric
    return {"L2": m.L2, "Cosine": m.Cosine, "InnerProduct": m.InnerProduct}


def _store_and_seeds(rng, d, n_store=N_STORE, n_seeds=N_SEEDS):
    keys = STORE_KEY0 + 3 * rng.permutation(n_store).astype(np.int64)
    rows = rng.standard_normal((n_store, d)).astype(np.float32)
    seeds = keys[rng.integers(0, n_store, n_seeds)]
    absent = rng.random(n_seeds) < 0.10
    seeds[absent] += 1                                  # 3 j + 1: no such key
    seeds[100:200] = seeds[0:100]                       # repeats, present and absent ones alike
    return keys, rows, seeds


def _host_composition(search, keys, rows, seeds, k):
    """QueryableByIdImplementation on the host: (seed, id, distance) triples, counts (-1 = absent)."""
    row_of = dict(zip(keys.tolist(), range(len(keys))))
    o_seed, o_id, o_dist, counts, memo = [], [], [], [], {}
    for s in seeds.tolist():
        r = row_of.get(s)
        if r is None:
            counts.append(-1)
            continue
        if s not in memo:  # (a repeated seed is the same search again)
            ids, dist, cnt = search(rows[r][None])
            memo[s] = (ids[0, :cnt[0]].copy(), dist[0, :cnt[0]].copy())
        ids, dist = memo[s]
        counts.append(len(ids))
        o_seed.append(np.full(len(ids), s, np.int64)); o_id.append(ids); o_dist.append(dist)
    cat = lambda a, t: np.concatenate(a) if a else np.zeros(0, t)  # noqa: E731
    return cat(o_seed, np.int64), cat(o_id, np.int64), cat(o_dist, np.float32), np.asarray(counts, np.int32)


def _assert_equal(got, want, what):
    g_seed, g_id, g_dist, g_cnt = got
    w_seed, w_id, w_dist, w_cnt = want
    print(f"{what}: triples {len(g_seed)} (want {len(w_seed)}), absent {(g_cnt < 0).sum()} (want {(w_cnt < 0).sum()})")
    assert np.array_equal(g_cnt, w_cnt), what
    assert len(g_seed) == len(w_seed), what
    assert np.array_equal(g_seed, w_seed), what
    assert np.array_equal(g_id, w_id), what
    assert np.array_equal(g_dist.view(np.uint32), w_dist.view(np.uint32)), what


def _check_seed_list(keys, seeds):
    present = np.isin(seeds, keys)
    n_absent = int((~present).sum())
    assert 0 < n_absent < len(seeds)
    assert len(np.unique(seeds)) < len(seeds)
    return n_absent


@pytest.mark.parametrize("d", [64, 200, 256])
@pytest.mark.parametrize("metric", ["L2", "Cosine", "InnerProduct"])
def test_hnsw_by_id_equals_the_host_composition(pkg, metric, d):
    m = _metrics(pkg)[metric]
    rng = np.random.default_rng(1000 + d + int(m))
    x = rng.standard_normal((N_INDEX, d)).astype(np.float32)
    ix = pkg.hnsw_ann.Hnsw.build(m, x, 5 + 7 * np.arange(N_INDEX, dtype=np.int64), max_m=16, ef_construction=100, seed=3, gpu=True)
    keys, rows, seeds = _store_and_seeds(rng, d)
    n_absent = _check_seed_list(keys, seeds)
    store = pkg.EmbeddingStore.build(keys, rows)
    q = pkg.QueryableById(store, ix)
    for k, ef in ((10, 100), (200, 800)):
        got = q.batch_arrays(seeds, k, pkg.hnsw_ann.HnswParams(ef))
        st = q.last_stats()
        want = _host_composition(lambda r: ix.search(r, k, ef), keys, rows, seeds, k)
        _assert_equal(got, want, f"hnsw {metric} d={d} k={k} ef={ef}")
        assert st["absent"] == n_absent and st["found"] == N_SEEDS - n_absent
    store.close(); ix.close()


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("metric", ["L2", "Cosine", "InnerProduct"])
def test_brute_force_by_id_equals_the_host_composition(pkg, metric, d, exact):
    m = _metrics(pkg)[metric]
    rng = np.random.default_rng(2000 + d + int(m))
    x = rng.standard_normal((N_INDEX, d)).astype(np.float32)
    ix = pkg.dense_ann.BruteForceIndex.build(m, x, 5 + 7 * np.arange(N_INDEX, dtype=np.int64), exact=exact)
    keys, rows, seeds = _store_and_seeds(rng, d)
    n_absent = _check_seed_list(keys, seeds)
    store = pkg.EmbeddingStore.build(keys, rows)
    q = pkg.QueryableById(store, ix)
    for k in (10, 200):
        got = q.batch_arrays(seeds, k)
        st = q.last_stats()
        want = _host_composition(lambda r: ix.search(r, k), keys, rows, seeds, k)
        _assert_equal(got, want, f"brute force {metric} d={d} exact={exact} k={k}")
        assert st["absent"] == n_absent and st["found"] == N_SEEDS - n_absent
    store.close(); ix.close()


def test_edge_cases(pkg):
    M = pkg.dense_ann.DistanceMetric
    rng = np.random.default_rng(7)
    d = 64
    x = rng.standard_normal((3000, d)).astype(np.float32)
    hn = pkg.hnsw_ann.Hnsw.build(M.Cosine, x, max_m=8, ef_construction=40, seed=5, gpu=True)
    bf = pkg.dense_ann.BruteForceIndex.build(M.Cosine, x)
    keys = np.arange(100, 600, dtype=np.int64)
    rows = rng.standard_normal((500, d)).astype(np.float32)
    rows[17] = 0.0  # Cosine: the preparation's norm = 1 branch
    store = pkg.EmbeddingStore.build(keys, rows)
    P = pkg.hnsw_ann.HnswParams(60)
    for q, search in ((pkg.QueryableById(store, hn), lambda r, k: hn.search(r, k, 60)), (pkg.QueryableById(store, bf), lambda r, k: bf.search(r, k))):
        # all seeds absent
        s, i, dist, cnt = q.batch_arrays(np.arange(5, dtype=np.int64), 10, P)
        assert len(s) == len(i) == len(dist) == 0 and (cnt == -1).all() and len(cnt) == 5
        assert q.last_stats()["found"] == 0 and q.last_stats()["absent"] == 5
        # one seed; the all-zero row
        for seeds in (np.array([300], np.int64), np.array([117], np.int64), np.array([117, 5, 118], np.int64)):
            _assert_equal(q.batch_arrays(seeds, 10, P), _host_composition(lambda r: search(r, 10), keys, rows, seeds, 10), f"seeds {seeds}")
        # the four reference methods are views of the one call
        full = q.batchQueryWithDistanceById([300, 5, 301], 4, P)
        assert [t[0] for t in full] == [300] * 4 + [301] * 4
        assert q.batchQueryById([300, 5, 301], 4, P) == [t[:2] for t in full]
        assert q.queryByIdWithDistance(300, 4, P) == [t[1:] for t in full[:4]] and q.queryById(301, 4, P) == [t[1] for t in full[4:]]
        assert q.queryById(5, 4, P) == []
        # a cap below n_found * k is refused, naming both; nothing is written beyond out_total when it is enough
        with pytest.raises(pkg.ann_by_id.AnnByIdError, match="cap 19 is below"):
            q.batch_arrays(np.array([300, 5, 301], np.int64), 10, P, cap=19)
        s, i, dist, cnt = q.batch_arrays(np.array([300, 5, 301], np.int64), 10, P, cap=20)
        assert len(s) == 20 and cnt.tolist() == [10, -1, 10]
    # k > n
    small = rng.standard_normal((7, d)).astype(np.float32)
    hs = pkg.hnsw_ann.Hnsw.build(M.L2, small, max_m=8, ef_construction=40, seed=5)
    bs = pkg.dense_ann.BruteForceIndex.build(M.L2, small)
    seeds = np.array([100, 101, 99, 102], np.int64)
    for q, search in ((pkg.QueryableById(store, hs), lambda r: hs.search(r, 50, 60)), (pkg.QueryableById(store, bs), lambda r: bs.search(r, 50))):
        got = q.batch_arrays(seeds, 50, P)
        _assert_equal(got, _host_composition(search, keys, rows, seeds, 50), "k > n")
        assert got[3].tolist() == [7, 7, -1, 7]
        st = q.last_stats()  # the triples copied back are out_total, not n_found * k padded rows
        assert st["d2h_result_bytes"] == 20 * 21 + 4 * 4 and st["d2h_bytes"] < 12 * 3 * 50
    # an empty HNSW graph: found seeds answer nothing, absent ones stay -1
    he = pkg.hnsw_ann.Hnsw.from_graph(M.L2, small, (np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, np.int64), -1, 0),
                                      max_m=8)
    s, i, dist, cnt = pkg.QueryableById(store, he).batch_arrays(seeds, 5, P)
    assert len(s) == 0 and cnt.tolist() == [0, 0, -1, 0]
    # refusals with the plain search's codes; the index is untouched
    other = pkg.EmbeddingStore.build(keys, rng.standard_normal((500, 32)).astype(np.float32))
    q = pkg.QueryableById(store, hn)
    q.store = other  # (past the wrapper's own check, to the library's)
    with pytest.raises(pkg.ann_by_id.AnnByIdError, match="error 1: the store holds rows of dimension 32"):
        q.batch_arrays(seeds, 5, P)
    q.store = store
    with pytest.raises(pkg.ann_by_id.AnnByIdError, match="error 3: .*1024"):
        q.batch_arrays(seeds, 5, pkg.hnsw_ann.HnswParams(2000))
    _assert_equal(q.batch_arrays(seeds, 5, P), _host_composition(lambda r: hn.search(r, 5, 60), keys, rows, seeds, 5), "after refusals")
    for o in (other, store, hn, bf, hs, bs, he):
        o.close()


@pytest.mark.parametrize("metric", ["L2", "Cosine", "InnerProduct"])
def test_the_index_as_its_own_producer(pkg, metric):
    """store = None on indexes that were appended to and (HNSW) updated since their build: the key -> position table follows."""
    m = _metrics(pkg)[metric]
    rng = np.random.default_rng(300 + int(m))
    d, n0, n1 = 64, 4000, 1500
    x0, x1 = rng.standard_normal((n0, d)).astype(np.float32), rng.standard_normal((n1, d)).astype(np.float32)
    id0 = 1000 + 2 * rng.permutation(n0).astype(np.int64)
    id1 = 1001 + 2 * rng.permutation(n0 + n1)[:n1].astype(np.int64)  # odd: new keys, interleaved with the old ones
    absent = np.array([0, 7, 999, 10**12], np.int64)

    hn = pkg.hnsw_ann.Hnsw.build(m, x0, id0, max_m=8, ef_construction=40, seed=5, gpu=True)
    q = pkg.QueryableById(None, hn)
    P = pkg.hnsw_ann.HnswParams(80)

    def check_hnsw(what):
        ids, stored = hn.ids(), hn.stored_vectors()
        seeds = np.concatenate([rng.choice(ids, 600), absent, ids[:50]])
        rng.shuffle(seeds)
        _assert_equal(q.batch_arrays(seeds, 10, P), _host_composition(lambda r: hn.search(r, 10, 80), ids, stored, seeds, 10), what)

    check_hnsw(f"hnsw own keys {metric}: built")
    hn.append(x1, id1, ef_construction=40, seed=5)
    check_hnsw(f"hnsw own keys {metric}: appended")
    upd = rng.choice(np.concatenate([id0, id1]), 300, replace=False)
    assert hn.update(rng.standard_normal((300, d)).astype(np.float32), upd, ef_construction=40, seed=5) == 0
    check_hnsw(f"hnsw own keys {metric}: updated")
    hn.close()
    # an index created without ids: its keys are positions
    hp = pkg.hnsw_ann.Hnsw.build(m, x0, max_m=8, ef_construction=40, seed=5, gpu=True)
    seeds = np.array([5, n0, 0, -1, n0 - 1, 5], np.int64)
    _assert_equal(pkg.QueryableById(None, hp).batch_arrays(seeds, 10, P),
                  _host_composition(lambda r: hp.search(r, 10, 80), np.arange(n0, dtype=np.int64), hp.stored_vectors(), seeds, 10), "hnsw positions")
    hp.close()

    for exact in (False, True):
        bf = pkg.dense_ann.BruteForceIndex.build(m, x0, id0, exact=exact)
        qb = pkg.QueryableById(None, bf)

        def check_dense(ids_by_pos, what):
            stored = bf.stored_vectors()
            seeds = np.concatenate([rng.choice(ids_by_pos, 600), absent, ids_by_pos[:50]])
            rng.shuffle(seeds)
            _assert_equal(qb.batch_arrays(seeds, 10), _host_composition(lambda r: bf.search(r, 10), ids_by_pos, stored, seeds, 10), what)

        check_dense(np.sort(id0), f"brute force own keys {metric} exact={exact}: built")  # a build stores its rows in id order
        bf.append(x1, id1)                                                                 # ... and an append its own, after them
        check_dense(np.concatenate([np.sort(id0), np.sort(id1)]), f"brute force own keys {metric} exact={exact}: appended")
        bf.close()
    bp = pkg.dense_ann.BruteForceIndex.build(m, x0)
    _assert_equal(pkg.QueryableById(None, bp).batch_arrays(seeds, 10),
                  _host_composition(lambda r: bp.search(r, 10), np.arange(n0, dtype=np.int64), bp.stored_vectors(), seeds, 10), "brute force positions")
    bp.close()


def test_hnsw_spill_path_by_id(pkg):
    """The second pass (redo / qlist) of the walk serves by-id queries as it serves plain ones (HNSW_DEBUG_CCAP as in test_hnsw_gpu.py)."""
    m = pkg.dense_ann.DistanceMetric.L2
    rng = np.random.default_rng(11)
    x = rng.standard_normal((3000, 64)).astype(np.float32)
    ix = pkg.hnsw_ann.Hnsw.build(m, x, max_m=8, ef_construction=40, seed=5, gpu=True)
    keys, rows, seeds = _store_and_seeds(rng, 64, n_store=500, n_seeds=200)
    store = pkg.EmbeddingStore.build(keys, rows)
    q = pkg.QueryableById(store, ix)
    P = pkg.hnsw_ann.HnswParams(1024)
    plain = q.batch_arrays(seeds, 100, P)
    n_found = int((plain[3] >= 0).sum())
    assert q.last_stats()["h2d_bytes"] == 8 * len(seeds) + 4 * ix.last_stats()["spilled_queries"]
    os.environ["HNSW_DEBUG_CCAP"] = "40"
    try:
        got = q.batch_arrays(seeds, 100, P)
        assert ix.last_stats()["spilled_queries"] == n_found
        assert q.last_stats()["h2d_bytes"] == 8 * len(seeds) + 4 * n_found  # the second pass's query list, as in the plain search
        _assert_equal(got, plain, "spill, CCAP 40")
        _assert_equal(got, _host_composition(lambda r: ix.search(r, 100, 1024), keys, rows, seeds, 100), "spill vs the plain search")
        os.environ["HNSW_DEBUG_CCAP"] = "-7"
        _assert_equal(q.batch_arrays(seeds, 100, P), plain, "spill, CCAP -7")
    finally:
        del os.environ["HNSW_DEBUG_CCAP"]
    store.close(); ix.close()


def test_no_embedding_crosses_the_bus(pkg):
    M = pkg.dense_ann.DistanceMetric
    rng = np.random.default_rng(13)
    d, n_seeds, k = 256, 1000, 10
    x = rng.standard_normal((5000, d)).astype(np.float32)
    keys, rows, seeds = _store_and_seeds(rng, d, n_store=4000, n_seeds=n_seeds)
    store = pkg.EmbeddingStore.build(keys, rows)
    hn = pkg.hnsw_ann.Hnsw.build(M.Cosine, x, max_m=8, ef_construction=40, seed=5, gpu=True)
    for exact in (False, True):
        bf = pkg.dense_ann.BruteForceIndex.build(M.Cosine, x, exact=exact)
        q = pkg.QueryableById(store, bf)
        s, i, dist, cnt = q.batch_arrays(seeds, k)
        st = q.last_stats()
        print("brute force exact =", exact, st)
        assert st["h2d_bytes"] == 8 * n_seeds                                   # the seed ids and nothing else
        assert st["d2h_result_bytes"] == 20 * len(s) + 4 * n_seeds
        ctl, rounds = st["d2h_bytes"] - st["d2h_result_bytes"], bf.last_rounds()  # n_found, out_total, and the rounds' flags
        assert 8 + 4 * rounds + (4 if exact else 0) <= ctl <= 8 + 4 * (2 if exact else 1) * rounds
        assert st["h2d_bytes"] + st["d2h_bytes"] < st["found"] * d * 4          # below the size of the embeddings alone
        bf.close()
    q = pkg.QueryableById(store, hn)
    s, i, dist, cnt = q.batch_arrays(seeds, k, pkg.hnsw_ann.HnswParams(50))
    st = q.last_stats()
    print("hnsw", st)
    assert hn.last_stats()["spilled_queries"] == 0
    assert st["h2d_bytes"] == 8 * n_seeds
    assert st["d2h_result_bytes"] == 20 * len(s) + 4 * n_seeds
    assert st["d2h_bytes"] - st["d2h_result_bytes"] == 8 + 128 + 4 * st["found"]
    assert st["resolve_gather_ms"] > 0 and st["search_ms"] > 0 and st["flatten_ms"] > 0
    store.close(); hn.close()


def test_store_refuses_a_repeated_key_and_returns_rows_bit_for_bit(pkg):
    rng = np.random.default_rng(17)
    for d in (7, 64, 200):
        keys = rng.permutation(10**6)[:3000].astype(np.int64) - 500000
        rows = rng.standard_normal((3000, d)).astype(np.float32)
        rows[5, 0] = np.float32("nan"); rows[6, 1] = -0.0
        store = pkg.EmbeddingStore.build(keys, rows)
        ask = np.concatenate([keys[::-3], np.array([10**7, -(10**7)], np.int64), keys[:3]])
        got, found = store.get(ask)
        assert found.tolist() == [True] * len(keys[::-3]) + [False, False] + [True] * 3
        want = np.concatenate([rows[::-3], np.zeros((2, d), np.float32), rows[:3]])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        store.close()
    bad = keys.copy()
    bad[1234] = bad[77]
    with pytest.raises(pkg.ann_by_id.AnnByIdError, match=f"duplicate key {bad[77]}:"):
        pkg.EmbeddingStore.build(bad, rows)
    empty = pkg.EmbeddingStore.build(np.zeros(0, np.int64), np.zeros((0, 64), np.float32))
    assert not empty.get([1, 2])[1].any()
    empty.close()


def test_jni_round_trip(pkg):
    import _jni
    from _jni import ANN

    m = pkg.dense_ann.DistanceMetric.Cosine
    rng = np.random.default_rng(19)
    n, d, k, ef = 2000, 64, 10, 50
    x = rng.standard_normal((n, d)).astype(np.float32)
    keys, rows, seeds = _store_and_seeds(rng, d, n_store=800, n_seeds=300)
    e = _jni.Env()
    st, msg, _ = e.call(ANN, "embeddingStoreBuild", C.c_int64, 0, C.c_int64(len(keys)), d, e.buffer(keys), e.buffer(rows))
    assert msg is None and st
    h, msg, _ = e.call(ANN, "hnswIndexBuildInsert", C.c_int64, 0, int(m), C.c_int64(n), d, e.buffer(x), None, 8, 40, C.c_int64(5), 0)
    assert msg is None and h
    cap = len(seeds) * k
    o_seed, o_id, o_dist, cnt = np.zeros(cap, np.int64), np.zeros(cap, np.int64), np.zeros(cap, np.float32), np.zeros(len(seeds), np.int32)
    total, msg, _ = e.call(ANN, "hnswBatchQueryById", C.c_int64, C.c_int64(h), C.c_int64(st), len(seeds), e.buffer(seeds), k, ef, e.buffer(o_seed),
                           e.buffer(o_id), e.buffer(o_dist), C.c_int64(cap), e.buffer(cnt))
    assert msg is None
    ix = pkg.hnsw_ann.Hnsw.build(m, x, max_m=8, ef_construction=40, seed=5, gpu=True)
    store = pkg.EmbeddingStore.build(keys, rows)
    want = pkg.QueryableById(store, ix).batch_arrays(seeds, k, pkg.hnsw_ann.HnswParams(ef))
    assert total == len(want[0]) > 0
    _assert_equal((o_seed[:total], o_id[:total], o_dist[:total], cnt), want, "jni hnsw")
    assert not o_seed[total:].any() and not o_dist[total:].any()  # nothing beyond out_total
    hb, msg, _ = e.call(ANN, "denseIndexBuild", C.c_int64, 0, int(m), C.c_int64(n), d, e.buffer(x), None, False)
    assert msg is None and hb
    total, msg, _ = e.call(ANN, "denseBatchQueryById", C.c_int64, C.c_int64(hb), C.c_int64(st), len(seeds), e.buffer(seeds), k, e.buffer(o_seed),
                           e.buffer(o_id), e.buffer(o_dist), C.c_int64(cap), e.buffer(cnt))
    assert msg is None
    bf = pkg.dense_ann.BruteForceIndex.build(m, x)
    want = pkg.QueryableById(store, bf).batch_arrays(seeds, k)
    _assert_equal((o_seed[:total], o_id[:total], o_dist[:total], cnt), want, "jni brute force")
    total, msg, _ = e.call(ANN, "hnswBatchQueryById", C.c_int64, C.c_int64(h), C.c_int64(st), len(seeds), e.buffer(seeds), k, ef, e.buffer(o_seed),
                           e.buffer(o_id), e.buffer(o_dist), C.c_int64(cap), e.buffer(cnt[:-1]))
    assert total == 0 and "smaller than" in msg
    e.call(ANN, "hnswIndexDestroy", None, C.c_int64(h)); e.call(ANN, "denseIndexDestroy", None, C.c_int64(hb))
    e.call(ANN, "embeddingStoreDestroy", None, C.c_int64(st))
    for o in (ix, store, bf):
        o.close()
