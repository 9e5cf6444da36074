"""Hnsw.append on the device (hnsw_index_append): the device builder's rounds continued on a live index.

The yardstick is the UNCHANGED oracle of the builder: with every appended row at level 0 and the base size on a round boundary
of the builder's schedule, order(X0 ++ X1) is order(X0) ++ X1 and the rounds of a build of X0 ++ X1 are those of the build of
X0 followed by those of the append -- so the grown graph must be oracle_hnsw_build_batched(X0 ++ X1) entry for entry."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _levels_of(graph, n):
    lv, it = graph[0], graph[1]
    out = np.zeros(n, np.int32)
    np.maximum.at(out, it, lv)
    out[graph[4]] = graph[5]
    return out


def _same_graph(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4] and a[5] == b[5]


def _boundaries(n, batch):
    """Round boundaries of the builder's schedule: b0 = 1, b_{i+1} = b_i + min(batch, max(1, b_i // 8))."""
    out, b = [1], 1
    while b < n:
        b += min(batch, max(1, b // 8))
        out.append(b)
    return out


def _draw_levels(rng, n, max_m):
    u = 1.0 - rng.random(n)
    return np.minimum(60, (-np.log(u) / np.log(max_m)).astype(np.int32)).astype(np.int32)


def _well_formed(g, n, max_m):
    lv, it, off, nb = g[:4]
    sizes = np.diff(off)
    assert (lv == 0).sum() >= n - 1 and set(it[lv == 0].tolist()) >= set(range(n)) - {g[4]}, "every row has a layer-0 key"
    assert sizes[lv == 0].max() <= 2 * max_m and (sizes[lv > 0].max() if (lv > 0).any() else 0) <= max_m
    for e in range(len(lv)):
        row = nb[off[e]:off[e + 1]]
        assert it[e] not in row and len(set(row.tolist())) == len(row), "no self loops, no repeated neighbour"
    assert nb.max(initial=0) < n


SHAPES = [("L2", 3000, 24, 6, 40, 256), ("Cosine", 2500, 70, 8, 64, 128), ("InnerProduct", 2000, 16, 4, 16, 512),
          ("L2", 1500, 8, 2, 256, 64)]


@pytest.mark.parametrize("metric,n,d,max_m,efc,batch", SHAPES)
def test_append_is_the_batched_oracles_graph(pkg, oracle, metric, n, d, max_m, efc, batch):
    m = getattr(pkg.dense_ann.DistanceMetric, metric)
    rng = np.random.default_rng(n + d + 1)
    x = rng.standard_normal((n, d)).astype(np.float32)
    bounds = _boundaries(n, batch)
    n0 = max(b for b in bounds if b <= int(n * 0.6))
    x[n0 + 3] = x[n0 // 3]  # equal rows across the base and the append
    x[n0 + 4] = x[n0 // 3]
    x[n0 + 5] = x[n0 + 6]
    l0 = _draw_levels(rng, n0, max_m)
    assert l0.max() >= 2
    levels = np.concatenate([l0, np.zeros(n - n0, np.int32)])
    Hnsw = pkg.hnsw_ann.Hnsw
    ix = Hnsw.build(m, x[:n0], max_m=max_m, ef_construction=efc, levels=l0, gpu=True, batch=batch)
    try:
        ix.append(x[n0:], ef_construction=efc, levels=np.zeros(n - n0, np.int32), batch=batch)
        assert ix.n == n
        stored = ix.stored_vectors()
        want = oracle.hnsw_build_batched(int(m), stored, levels, max_m, efc, batch)
        g = ix.graph()
        assert g[4] == want[4] and g[5] == want[5], "entry point / max level"
        assert np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1]), "the same HnswNode(level, item) keys"
        assert np.array_equal(g[2], want[2]) and np.array_equal(g[3], want[3]), "the same lists, in the same order"
        rounds, unseen, _, dropped = ix.build_stats()  # the last append's rounds: the schedule's from n0 on
        assert rounds == sum(1 for b in bounds if n0 < b < n) + 1 and unseen == 0 and dropped == 0
    finally:
        ix.close()
    # the same with X1 split into several appends, each ending on a round boundary
    cuts = [b for b in bounds if n0 < b < n][::3] + [n]
    ix = Hnsw.build(m, x[:n0], max_m=max_m, ef_construction=efc, levels=l0, gpu=True, batch=batch)
    try:
        at = n0
        for c in cuts:
            ix.append(x[at:c], ef_construction=efc, levels=np.zeros(c - at, np.int32), batch=batch)
            at = c
        assert _same_graph(ix.graph(), want)
    finally:
        ix.close()
    # load a directory (here: the oracle's graph of X0), then append
    g0 = oracle.hnsw_build_batched(int(m), stored[:n0], l0, max_m, efc, batch)
    ix = Hnsw.from_graph(m, x[:n0], g0, max_m=max_m)
    try:
        ix.append(x[n0:], ef_construction=efc, levels=np.zeros(n - n0, np.int32), batch=batch)
        assert _same_graph(ix.graph(), want)
    finally:
        ix.close()


def test_a_large_append_is_the_batched_oracles_graph(pkg, oracle):
    m = pkg.dense_ann.DistanceMetric.L2
    rng = np.random.default_rng(2024)
    n, d, max_m, efc, batch = 150_000, 16, 6, 24, 4096
    x = rng.standard_normal((n, d)).astype(np.float32)
    n0 = max(b for b in _boundaries(n, batch) if b <= 120_000)
    l0 = _draw_levels(rng, n0, max_m)
    ix = pkg.hnsw_ann.Hnsw.build(m, x[:n0], max_m=max_m, ef_construction=efc, levels=l0, gpu=True, batch=batch)
    try:
        ix.append(x[n0:], ef_construction=efc, levels=np.zeros(n - n0, np.int32), batch=batch)
        want = oracle.hnsw_build_batched(int(m), ix.stored_vectors(), np.concatenate([l0, np.zeros(n - n0, np.int32)]), max_m, efc, batch)
        assert _same_graph(ix.graph(), want)
    finally:
        ix.close()


@pytest.mark.parametrize("keyed", [False, True])
def test_append_to_an_empty_index_is_a_build(pkg, keyed):
    m = pkg.dense_ann.DistanceMetric.Cosine
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1200, 32)).astype(np.float32)
    lv = _draw_levels(rng, 1200, 8)
    keys = np.arange(1200, dtype=np.int64) * 5 + 1 if keyed else None
    Hnsw = pkg.hnsw_ann.Hnsw
    empty = Hnsw.build(m, x[:0], ids=None if keys is None else keys[:0], max_m=8, ef_construction=50, levels=lv[:0], gpu=True, batch=128)
    full = Hnsw.build(m, x, ids=keys, max_m=8, ef_construction=50, levels=lv, gpu=True, batch=128)
    try:
        assert empty.n == 0
        empty.append(x, keys, ef_construction=50, levels=lv, batch=128)
        assert empty.n == 1200
        assert _same_graph(empty.graph(), full.graph())
        q = rng.standard_normal((30, 32)).astype(np.float32)
        assert all(np.array_equal(a, b) for a, b in zip(empty.search(q, 10, 40), full.search(q, 10, 40)))
    finally:
        empty.close(); full.close()


def test_rows_above_max_level_move_the_entry_point(pkg, oracle):
    m = pkg.dense_ann.DistanceMetric.L2
    rng = np.random.default_rng(41)
    n0, n1, d, max_m = 4000, 1500, 24, 8
    x = rng.standard_normal((n0 + n1, d)).astype(np.float32)
    l0 = np.minimum(_draw_levels(rng, n0, max_m), 2)
    l0[17] = 2
    l1 = np.minimum(_draw_levels(rng, n1, max_m), 2)
    l1[5] = 4
    l1[9] = 4  # the same round as row 5 (the first round of the append): the first in order wins
    l1[900] = 3  # the second append: wired on layer 3 from the new entry point

    def grown():
        ix = pkg.hnsw_ann.Hnsw.build(m, x[:n0], max_m=max_m, ef_construction=60, levels=l0, gpu=True, batch=256)
        ix.append(x[n0:n0 + 800], ef_construction=60, levels=l1[:800], batch=256)
        ix.append(x[n0 + 800:], ef_construction=60, levels=l1[800:], batch=256)
        return ix

    a, b = grown(), grown()
    try:
        g = a.graph()
        assert g[4] == n0 + 5 and g[5] == 4
        _well_formed(g, n0 + n1, max_m)
        lv, it = g[0], g[1]
        assert set(it[lv == 3].tolist()) == {n0 + 5, n0 + 900} and (lv == 4).sum() == 0
        assert _same_graph(g, b.graph()), "two identical append sequences give one graph"
        stored = a.stored_vectors()
        q = rng.standard_normal((24, d)).astype(np.float32)
        ids, dist, cnt = a.search(q, 10, 50)
        pq = oracle.dense_prepare(int(m), q)
        for i in range(24):
            o_items, o_dist, _ = oracle.hnsw_search(int(m), stored, g, pq[i], 10, 50)
            assert np.array_equal(ids[i, :cnt[i]], o_items) and np.array_equal(dist[i, :cnt[i]].view(np.int32), o_dist.view(np.int32))
    finally:
        a.close(); b.close()


def test_grown_index_recalls_like_a_one_shot_build(pkg):
    m = pkg.dense_ann.DistanceMetric.Cosine
    rng = np.random.default_rng(8)
    centres = rng.standard_normal((200, 48)).astype(np.float32) * 2.0
    n = 40_000
    x = (centres[rng.integers(0, 200, n)] + rng.standard_normal((n, 48)).astype(np.float32) * 0.6).astype(np.float32)
    q = (centres[rng.integers(0, 200, 200)] + rng.standard_normal((200, 48)).astype(np.float32) * 0.6).astype(np.float32)
    bf = pkg.dense_ann.BruteForceIndex.build(m, x)
    t_ids, _, _ = bf.search(q, 10)
    bf.close()

    def recall(ix):
        ids, _, cnt = ix.search(q, 10, 100)
        return float(np.mean([len(set(ids[i, :cnt[i]]) & set(t_ids[i])) / 10 for i in range(len(q))]))

    one = pkg.hnsw_ann.Hnsw.build(m, x, max_m=12, ef_construction=100, seed=4, gpu=True)
    grown = pkg.hnsw_ann.Hnsw.build(m, x[:n // 2], max_m=12, ef_construction=100, seed=4, gpu=True)
    try:
        g0 = grown.graph()
        for at in range(n // 2, n, 3000):
            grown.append(x[at:at + 3000], ef_construction=100, seed=4)
        r1, r2 = recall(one), recall(grown)
        assert r1 > 0.9 and r2 > r1 - 0.03, (r1, r2)
        # the seeded draw at global positions: the levels of the one-shot build (below the base's top layer)
        lo, lg = _levels_of(one.graph(), n), _levels_of(grown.graph(), n)
        sel = lo <= g0[5]  # (a row above the base's top layer is wired only up to it)
        sel[[one.graph()[4], g0[4]]] = False  # (entry points have keys only where back links reached them)
        assert sel.sum() > n - 50 and np.array_equal(lo[sel], lg[sel])
    finally:
        one.close(); grown.close()


def test_drawn_levels_are_the_builders_at_global_positions(pkg):
    m = pkg.dense_ann.DistanceMetric.L2
    rng = np.random.default_rng(12)
    n, n0 = 6000, 4000
    x = rng.standard_normal((n, 16)).astype(np.float32)
    full = pkg.hnsw_ann.Hnsw.build(m, x, max_m=4, ef_construction=32, seed=77, gpu=True, batch=256)
    part = pkg.hnsw_ann.Hnsw.build(m, x[:n0], max_m=4, ef_construction=32, seed=77, gpu=True, batch=256)
    try:
        g0 = part.graph()
        part.append(x[n0:], ef_construction=32, seed=77, batch=256)
        lf, lp = _levels_of(full.graph(), n), _levels_of(part.graph(), n)
        sel = lf <= g0[5]  # a row above the base's top layer is wired only up to it
        sel[[full.graph()[4], g0[4]]] = False
        assert sel.sum() > n - 20 and np.array_equal(lf[sel], lp[sel])
    finally:
        full.close(); part.close()


def test_duplicate_keys_and_wrong_inputs_leave_the_index_unchanged(pkg):
    m = pkg.dense_ann.DistanceMetric.L2
    Hnsw, HnswError = pkg.hnsw_ann.Hnsw, pkg.hnsw_ann.HnswError
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3000, 32)).astype(np.float32) * 4
    keys = rng.permutation(100_000)[:3000].astype(np.int64) * 3 - 7
    q = rng.standard_normal((20, 32)).astype(np.float32)
    ix = Hnsw.build(m, x[:2000], ids=keys[:2000], max_m=8, ef_construction=60, seed=1, gpu=True)
    plain = Hnsw.build(m, x[:2000], max_m=8, ef_construction=60, seed=1, gpu=True)
    try:
        g, r = ix.graph(), ix.search(q, 10, 50)

        def unchanged():
            assert ix.n == 2000 and _same_graph(ix.graph(), g)
            assert all(np.array_equal(a, b) for a, b in zip(ix.search(q, 10, 50), r))

        bad = keys[2000:2100].copy()
        bad[37] = keys[1234]
        with pytest.raises(HnswError, match=f"duplicate key {keys[1234]}.*already in the index"):
            ix.append(x[2000:2100], bad)
        unchanged()
        bad = keys[2000:2100].copy()
        bad[60] = bad[10]
        with pytest.raises(HnswError, match=f"duplicate key {bad[10]}.*twice"):
            ix.append(x[2000:2100], bad)
        unchanged()
        with pytest.raises(HnswError, match="ids"):
            ix.append(x[2000:2100])
        unchanged()
        with pytest.raises(HnswError, match="ids"):
            plain.append(x[2000:2100], keys[2000:2100])
        assert plain.n == 2000
        with pytest.raises(ValueError):
            ix.append(x[2000:2100, :16], keys[2000:2100])
        with pytest.raises(HnswError):
            ix.append(x[2000:2100], keys[2000:2100], levels=np.full(100, 61, np.int32))
        with pytest.raises(HnswError):
            ix.append(x[2000:2100], keys[2000:2100], ef_construction=300)
        unchanged()
        # with ids: the appended keys come back from search
        ix.append(x[2000:], keys[2000:], ef_construction=60)
        ids, _, _ = ix.search(x[2000:2200] + 1e-3, 1, 64)
        assert np.mean(ids[:, 0] == keys[2000:2200]) > 0.97
        assert np.array_equal(ix.ids(), keys)
        with pytest.raises(HnswError, match=f"duplicate key {keys[2500]}"):
            ix.append(x[:1], keys[2500:2501])  # a key of an earlier append: the merged table holds it
    finally:
        ix.close(); plain.close()


def test_many_small_appends_cross_capacity_steps(pkg, oracle, monkeypatch):
    monkeypatch.setenv("HNSW_DEBUG_VLOG", "1")  # the undo log of large indexes: searches across growth start on clean bitmaps
    m = pkg.dense_ann.DistanceMetric.L2
    Hnsw = pkg.hnsw_ann.Hnsw
    rng = np.random.default_rng(99)
    sizes = rng.integers(1, 65, 200)
    n0 = 500
    n = n0 + int(sizes.sum())
    x = rng.standard_normal((n, 32)).astype(np.float32) * 3
    keys = rng.permutation(10 * n)[:n].astype(np.int64)
    q = rng.standard_normal((16, 32)).astype(np.float32)
    ix = Hnsw.build(m, x[:n0], ids=keys[:n0], max_m=8, ef_construction=64, seed=2, gpu=True)
    try:
        before = ix.search(q, 10, 60)
        at, misses = n0, 0
        for step, s in enumerate(sizes):
            ix.append(x[at:at + s], keys[at:at + s], ef_construction=64, seed=2)
            at += int(s)
            assert ix.n == at
            ids, _, cnt = ix.search(x[at - s:at], 1, 256)
            misses += int((ids[:, 0] != keys[at - s:at]).sum())
            if step % 50 == 0:
                g, stored = ix.graph(), ix.stored_vectors()
                ids, dist, cnt = ix.search(q, 10, 60)
                pq = oracle.dense_prepare(int(m), q)
                for i in range(len(q)):
                    o_items, o_dist, _ = oracle.hnsw_search(int(m), stored, g, pq[i], 10, 60)
                    assert np.array_equal(ids[i, :cnt[i]], keys[o_items])
                    assert np.array_equal(dist[i, :cnt[i]].view(np.int32), o_dist.view(np.int32))
        # a row whose every in-link a later re-selection dropped is unreachable (the reference's graphs have such rows too):
        # the grown index may miss a few self-queries, no more than a one-shot build of the same rows does, give or take
        one = Hnsw.build(m, x, ids=keys, max_m=8, ef_construction=64, seed=2, gpu=True)
        try:
            ids, _, _ = one.search(x[n0:], 1, 256)
            misses_one = int((ids[:, 0] != keys[n0:]).sum())
        finally:
            one.close()
        assert ix.n == n and misses <= misses_one + (n - n0) // 500, (misses, misses_one)
        assert np.array_equal(ix.ids(), keys)
        want = oracle.dense_prepare(int(m), x)  # L2: the fp16 rounding of the rows
        assert np.array_equal(ix.stored_vectors(), want.astype(np.float16).astype(np.float32))
        assert not all(np.array_equal(a, b) for a, b in zip(before, ix.search(q, 10, 60)))
    finally:
        ix.close()
    # reserve, then append
    ix = Hnsw.build(m, x[:n0], ids=keys[:n0], max_m=8, ef_construction=64, seed=2, gpu=True)
    ref = Hnsw.build(m, x[:n0], ids=keys[:n0], max_m=8, ef_construction=64, seed=2, gpu=True)
    try:
        ix.reserve(n)
        ix.reserve(10)  # never shrinks
        for at in range(n0, n, 1000):
            ix.append(x[at:at + 1000], keys[at:at + 1000], ef_construction=64, seed=2)
            ref.append(x[at:at + 1000], keys[at:at + 1000], ef_construction=64, seed=2)
        assert ix.n == n and _same_graph(ix.graph(), ref.graph())
    finally:
        ix.close(); ref.close()


def test_save_after_appends_then_load(pkg, tmp_path):
    ac = pkg.ann_codec
    m = pkg.dense_ann.DistanceMetric.Cosine
    rng = np.random.default_rng(31)
    x = rng.standard_normal((5000, 40)).astype(np.float32)
    keys = np.arange(5000, dtype=np.int64) * 11 + 5
    ix = pkg.hnsw_ann.Hnsw.build(m, x[:3000], ids=keys[:3000], max_m=8, ef_construction=50, seed=6, gpu=True)
    try:
        for at in range(3000, 5000, 700):
            ix.append(x[at:at + 700], keys[at:at + 700], ef_construction=50, seed=6)
        d = str(tmp_path / "grown")
        ac.save_directory(ix, 50, d)
        back = ac.load_directory(m, x, d, ids=keys)
        try:
            assert _same_graph(back.graph(), ix.graph())
            q = rng.standard_normal((40, 40)).astype(np.float32)
            assert all(np.array_equal(a, b) for a, b in zip(back.search(q, 10, 60), ix.search(q, 10, 60)))
            # and the loaded index appends like the one it was saved from
            more = rng.standard_normal((300, 40)).astype(np.float32)
            mk = np.arange(300, dtype=np.int64) + 10**9
            back.append(more, mk, ef_construction=50, seed=6)
            ix.append(more, mk, ef_construction=50, seed=6)
            assert _same_graph(back.graph(), ix.graph())
        finally:
            back.close()
    finally:
        ix.close()
