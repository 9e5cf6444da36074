"""Hnsw.update on the device (hnsw_index_update) against the CPU restatement of its rounds (tests/hnsw_update_ref.c), entry for
entry, plus search after an update, upsert, refusals, quality on moved clusters and the JNI entry."""
import ctypes as C

import numpy as np
import pytest

import _hnsw_update_ref as ref
import _jni
from _jni import ANN

pytestmark = pytest.mark.gpu


def _draw_levels(rng, n, max_m):
    u = 1.0 - rng.random(n)
    return np.minimum(60, (-np.log(u) / np.log(max_m)).astype(np.int32)).astype(np.int32)


def _check_against_ref(ix, metric, max_m, efc, pos, new, batch):
    before, stored = ix.graph(), ix.stored_vectors()
    ix.update(new, pos, ef_construction=efc, batch=batch)
    after = ix.stored_vectors()
    assert np.array_equal(after[np.setdiff1d(np.arange(ix.n), pos)], stored[np.setdiff1d(np.arange(ix.n), pos)])
    want, ws = ref.update(metric, stored, before, max_m, efc, after[pos], pos, batch or 4096)
    got = ix.graph()
    assert got[4] == before[4] and got[5] == before[5], "an update never moves the entry point"
    assert ref.as_dict(got) == ref.as_dict(want), "the restated rounds' graph, entry for entry"
    st = ix.update_stats()
    assert (st["rounds"], st["relinks"], st["relinks_superseded"], st["additions_already_present"], st["lists_kept"]) == ws
    return got, after


# (metric, n, d, max_m, efc, updates, batch, builder)
CASES = [("L2", 2000, 24, 8, 40, 64, 1, "gpu"), ("Cosine", 2000, 40, 16, 60, 64, 1, "host"),
         ("InnerProduct", 20000, 16, 8, 32, 2000, 0, "gpu"), ("L2", 20000, 32, 16, 48, 2000, 4096, "gpu"),
         ("Cosine", 20000, 24, 8, 40, 2000, 0, "load")]


def _update_case(pkg, oracle, metric, n, d, max_m, efc, nu, batch, builder):
    m = getattr(pkg.dense_ann.DistanceMetric, metric)
    Hnsw = pkg.hnsw_ann.Hnsw
    rng = np.random.default_rng(n + d + max_m)
    x = rng.standard_normal((n, d)).astype(np.float32)
    levels = _draw_levels(rng, n, max_m)
    if builder == "gpu":
        ix = Hnsw.build(m, x, max_m=max_m, ef_construction=efc, levels=levels, gpu=True)
    elif builder == "host":
        ix = Hnsw.build(m, x, max_m=max_m, ef_construction=efc, levels=levels)
    else:  # hnsw_index_build of a graph with an empty list and a node whose top entry is below its drawn level
        g0 = oracle.hnsw_build_batched(int(m), oracle.dense_prepare(int(m), x), levels, max_m, efc)
        d0 = ref.as_dict(g0)
        upper = sorted(k for k in d0 if k[0] > 0 and k[1] != g0[4])
        cut = upper[-1]
        del d0[cut]  # its top key gone: exists below its drawn level only
        empty = next(k for k in sorted(d0) if k[0] == 0 and k[1] != g0[4])
        d0[empty] = []
        keys = sorted(d0)
        off = np.concatenate([[0], np.cumsum([len(d0[k]) for k in keys])]).astype(np.int64)
        g = (np.array([k[0] for k in keys], np.int32), np.array([k[1] for k in keys], np.int64), off,
             np.array(sum((d0[k] for k in keys), []), np.int64), g0[4], g0[5])
        ix = Hnsw.from_graph(m, x, g, max_m=max_m)
    try:
        g = ix.graph()
        special = [g[4]] + [int(i) for i in np.unique(g[1][g[0] > 0])[:8]]  # the entry point, rows at upper levels
        if builder == "load":
            special += [cut[1], empty[1]]
        special = list(dict.fromkeys(special))
        rest = [int(i) for i in rng.permutation(n) if int(i) not in set(special)]
        pos = np.array(special[:1] + rest[:nu - len(special)] + special[1:], np.int64)
        new = rng.standard_normal((nu, d)).astype(np.float32)
        got, stored = _check_against_ref(ix, int(m), max_m, efc, pos, new, batch)
        assert np.array_equal(stored[pos], oracle.dense_prepare(int(m), new)), "hnsw_index_get_vectors returns the new rows"
        # search after the update: the walk over the restated graph and the new rows
        q = rng.standard_normal((16, d)).astype(np.float32)
        ids, dist, cnt = ix.search(q, 10, 50)
        for r in range(len(q)):
            oi, od, _ = oracle.hnsw_search(int(m), stored, got, oracle.dense_prepare(int(m), q[r:r + 1])[0], 10, 50)
            assert cnt[r] == len(oi) and np.array_equal(ids[r, :cnt[r]], oi)
            assert np.array_equal(dist[r, :cnt[r]].view(np.int32), od.view(np.int32))
    finally:
        ix.close()


@pytest.mark.parametrize("metric,n,d,max_m,efc,nu,batch,builder", CASES)
def test_update_is_the_restated_graph(pkg, oracle, metric, n, d, max_m, efc, nu, batch, builder):
    _update_case(pkg, oracle, metric, n, d, max_m, efc, nu, batch, builder)


def test_update_with_the_undo_log_is_the_restated_graph(pkg, oracle, monkeypatch):
    """The first case again with the undo log of large indexes forced on (bitmaps of 1 MB and more keep one): the relink
    kernel then finds its bitmaps clean and does not wipe them, and the update's walks undo their own marks."""
    monkeypatch.setenv("HNSW_DEBUG_VLOG", "1")  # (read when the construction scratch is reserved: set before the build)
    _update_case(pkg, oracle, *CASES[0])


def test_upsert_is_update_then_append(pkg):
    m = pkg.dense_ann.DistanceMetric.L2
    Hnsw = pkg.hnsw_ann.Hnsw
    rng = np.random.default_rng(5)
    n, d = 3000, 32
    x = rng.standard_normal((n, d)).astype(np.float32)
    keys = rng.permutation(10 * n)[:n].astype(np.int64) + 7
    a, b = (Hnsw.build(m, x, ids=keys, max_m=8, ef_construction=40, seed=3, gpu=True) for _ in range(2))
    try:
        pk = keys[rng.permutation(n)[:300]]
        ak = np.arange(10 * n + 100, 10 * n + 400, dtype=np.int64)
        rows = rng.standard_normal((600, d)).astype(np.float32)
        mix = rng.permutation(600)
        allk = np.concatenate([pk, ak])[mix]
        allr = rows[mix]
        assert a.update(allr, allk, ef_construction=40, seed=9, batch=128) == 300
        in_p = np.isin(allk, pk)
        assert b.update(allr[in_p], allk[in_p], ef_construction=40, seed=9, batch=128) == 0
        b.append(allr[~in_p], allk[~in_p], ef_construction=40, seed=9, batch=128)
        assert a.n == b.n == n + 300
        assert ref.as_dict(a.graph()) == ref.as_dict(b.graph()) and a.graph()[4:] == b.graph()[4:]
        assert np.array_equal(a.ids(), b.ids()) and np.array_equal(a.stored_vectors(), b.stored_vectors())
        # keys are looked up again after the append: the appended keys are now present
        assert a.update(rows[:3], ak[:3], ef_construction=40) == 0
    finally:
        a.close()
        b.close()


def test_refusals_leave_the_index_unchanged(pkg):
    m = pkg.dense_ann.DistanceMetric.Cosine
    Hnsw = pkg.hnsw_ann.Hnsw
    HnswError = pkg.hnsw_ann.HnswError
    rng = np.random.default_rng(8)
    n, d = 1500, 16
    x = rng.standard_normal((n, d)).astype(np.float32)
    ix = Hnsw.build(m, x, max_m=8, ef_construction=30, gpu=True)
    ik = Hnsw.build(m, x, ids=np.arange(n, dtype=np.int64) * 3, max_m=8, ef_construction=30, gpu=True)
    try:
        for h in (ix, ik):
            g0, v0 = h.graph(), h.stored_vectors()
            r = rng.standard_normal((4, d)).astype(np.float32)
            bad = [(dict(ids=[0, 3, 6, 3]), "appears twice"), (dict(ids=[0, 3, 6, 9], ef_construction=0), "ef_construction"),
                   (dict(ids=[0, 3, 6, 9], ef_construction=257), "ef_construction"), (dict(ids=[0, 3, 6, 9], batch=-1), "batch"),
                   (dict(ids=[0, 3, 6, 9], batch=(1 << 20) + 1), "batch")]
            if h is ix:
                bad.append((dict(ids=[0, 1, 2, n]), "not in the index"))
            for kw, msg in bad:
                ids = kw.pop("ids")
                with pytest.raises(HnswError, match=msg):
                    h.update(r, ids, **kw)
                g1 = h.graph()
                assert all(np.array_equal(p, q) for p, q in zip(g0[:4], g1[:4])) and g0[4:] == g1[4:]
                assert np.array_equal(h.stored_vectors(), v0) and h.n == n
    finally:
        ix.close()
        ik.close()


def _recall(found, truth):
    return float(np.mean([len(set(f.tolist()) & set(t.tolist())) / len(t) for f, t in zip(found, truth)]))


def test_quality_after_moving_ten_percent(pkg, oracle):
    # Margins set from the measured runs on an MI355X: recall@10 (ef = 100) 0.9930 after the update at the default batch (4096;
    # 0.9950 at batch 1024), 0.9995 for a fresh build of the moved rows, 0.9030 for the old graph over the new rows (overwritten
    # without relinking).
    m = pkg.dense_ann.DistanceMetric.L2
    Hnsw = pkg.hnsw_ann.Hnsw
    rng = np.random.default_rng(21)
    n, d, k = 50000, 32, 64
    centres = rng.standard_normal((k, d)).astype(np.float32) * 4
    lab = rng.integers(0, k, n)
    x = centres[lab] + rng.standard_normal((n, d)).astype(np.float32)
    moved = rng.permutation(n)[:n // 10].astype(np.int64)
    y = x.copy()
    y[moved] = centres[(lab[moved] + 1 + rng.integers(0, k - 1, len(moved))) % k] + rng.standard_normal((len(moved), d)).astype(np.float32)
    q = centres[rng.integers(0, k, 200)] + rng.standard_normal((200, d)).astype(np.float32)
    yq = oracle.dense_prepare(0, y)
    qq = oracle.dense_prepare(0, q)
    dd = (yq * yq).sum(1)[None, :] - 2.0 * (qq @ yq.T)
    truth = np.argsort(dd, axis=1, kind="stable")[:, :10]
    ix = Hnsw.build(m, x, max_m=16, ef_construction=100, gpu=True)
    fresh = Hnsw.build(m, y, max_m=16, ef_construction=100, gpu=True)
    try:
        stale = Hnsw.from_graph(m, y, ix.graph(), max_m=16)  # the vectors overwritten, the old graph kept
        ix.update(y[moved], moved, ef_construction=100)
        r_upd = _recall(ix.search(q, 10, 100)[0], truth)
        r_fresh = _recall(fresh.search(q, 10, 100)[0], truth)
        r_stale = _recall(stale.search(q, 10, 100)[0], truth)
        stale.close()
        print(f"recall@10 ef=100: update {r_upd:.4f} fresh {r_fresh:.4f} overwrite-only {r_stale:.4f}")
        assert r_upd >= r_fresh - 0.03
        assert r_upd >= r_stale + 0.05
    finally:
        ix.close()
        fresh.close()


def test_jni_update_equals_the_c_call(pkg):
    e = _jni.Env()
    rng = np.random.default_rng(17)
    n, d = 3000, 32
    x = rng.standard_normal((n, d)).astype(np.float32)
    keys = rng.permutation(10 * n)[:n].astype(np.int64)
    m = pkg.dense_ann.DistanceMetric.L2
    h, msg, _ = e.call(ANN, "hnswIndexBuildInsert", C.c_int64, 0, int(m), C.c_int64(n), d, e.buffer(x), e.buffer(keys), 8, 60, C.c_int64(5), 0)
    assert msg is None and h
    py = pkg.hnsw_ann.Hnsw.build(m, x, ids=keys, max_m=8, ef_construction=60, seed=5, gpu=True)
    try:
        uk = np.concatenate([keys[rng.permutation(n)[:200]], np.array([10 * n + 1, 10 * n + 2], np.int64)])
        ur = rng.standard_normal((len(uk), d)).astype(np.float32)
        _, msg, _ = e.call(ANN, "hnswIndexUpdate", None, C.c_int64(h), C.c_int64(len(uk)), d, e.buffer(ur), e.buffer(uk), 60, C.c_int64(5))
        assert msg is None, msg
        assert py.update(ur, uk, ef_construction=60, seed=5) == 2
        q = rng.standard_normal((16, d)).astype(np.float32)
        dist, lab, cnt = np.zeros((16, 10), np.float32), np.zeros((16, 10), np.int64), np.zeros(16, np.int32)
        _, msg, _ = e.call(ANN, "hnswSearch", None, C.c_int64(h), 16, d, e.buffer(q), 10, 50, e.buffer(dist), e.buffer(lab), e.buffer(cnt))
        assert msg is None
        pi, pd, pc = py.search(q, 10, 50)
        assert np.array_equal(lab, pi) and np.array_equal(dist, pd) and np.array_equal(cnt, pc)
        _, msg, _ = e.call(ANN, "hnswIndexUpdate", None, C.c_int64(h), C.c_int64(1), 16, e.buffer(ur[:1]), e.buffer(uk[:1]), 60, C.c_int64(5))
        assert msg and "dimension" in msg
        _, msg, _ = e.call(ANN, "hnswIndexUpdate", None, C.c_int64(h), C.c_int64(2), d, e.buffer(ur[:2]), e.buffer(uk[[0, 0]]), 60, C.c_int64(5))
        assert msg and "twice" in msg
    finally:
        e.call(ANN, "hnswIndexDestroy", None, C.c_int64(h))
        py.close()
