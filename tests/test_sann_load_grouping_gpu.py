"""The grouped loads of desc_query_kernel and of the merge kernels' staging (score_deferred), at the edges of their slot
logic.  Every query of every case is compared with the oracle bit for bit (ids, score bits, count, map size).

Descriptor kernel.  A thread of desc_query_kernel resolves its sub-lists DESC_SLOTS = 8 at a time, every slot loading from
an item index clamped into the query's n_scan * P items.  The cases put n_scan * P at 0 (an empty embedding), below one
slot of 256 threads, at exactly one slot, one cluster over, at all eight slots (2048), and at the first size that needs
the second group (65 clusters, rows of 128) -- at P = 32 and P = 16 -- and run the one-wave-per-query instantiation
(P = 4, P = 8) with 1, 7 and 64 clusters.  (The smallest non-empty query at P = 32 has 32 items; 16 items is the
P = 16 case.)  The batch's last query scans the index's last row, whose last partition is non-empty in some cases and
empty in others: the clamped loads end exactly at the end of sub_offsets.  Lists are shorter than P (empty sub-lists),
shorter than M and longer than M.  The index caches cut tables for the first four distinct M it meets; the batch's last
two queries carry a fifth, which falls inside their sub-lists: their descriptors come from the search in `ranks`, the
path without a table.  Besides the answers, unit_T of every unit is compared with a host count.

Merge staging.  A thread of the merge kernel holds staged entry i in slot i / 256 and fetches the handed-over postings of
four slots per trip.  A unit that has no more live tweets than `keep_all` (sann_fast.hip) offers all of them, so a
query whose units all stay below that stages exactly as many entries as it has distinct tweets inside the window: the
designs put that number at <= 256, 257, 1024, 1025 and above the 1728 entries of one tournament round (and at the
matching edges of the 640-entry kernel and of merge_wave_kernel), and the test asserts it from cand_cnt.  Every query
mixes deferred entries, finished ones (tweets in two scanned clusters), a minScore that drops about half of them, and a
window that filters postings.  One offline case runs the norms fetch."""
import numpy as np
import pytest

import _sann_design as sd

pytestmark = pytest.mark.gpu

M_ALL = 20000
WINDOW_H = 12


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def _csr(lists):
    """lists: cluster id -> (ids, scores); ordered (score desc, id asc) per list, clusters ascending."""
    cids = sorted(lists)
    offs, tid, sc = [0], [], []
    for c in cids:
        ids, s = np.asarray(lists[c][0], np.int64), np.asarray(lists[c][1], np.float64)
        order = np.lexsort((ids, -s))
        tid.append(ids[order])
        sc.append(s[order])
        offs.append(offs[-1] + len(ids))
    tid = np.concatenate(tid) if tid else np.empty(0, np.int64)
    sc = np.concatenate(sc) if sc else np.empty(0, np.float64)
    return np.array(cids, np.int32), np.array(offs, np.int64), tid, sc


def _design(P, queries, lists, embs):
    cids, offs, tid, sc = _csr(lists)
    eo = np.zeros(len(embs) + 1, np.int64)
    eo[1:] = np.cumsum([len(e[0]) for e in embs])
    ec = np.concatenate([np.asarray(e[0], np.int32) for e in embs]) if embs else np.empty(0, np.int32)
    es = np.concatenate([np.asarray(e[1], np.float64) for e in embs]) if embs else np.empty(0, np.float64)
    return sd.Design(0, P, False, queries, cids, offs, tid, sc, eo, ec, es)


def _batch(pkg, d, index, cfgs, alg):
    pc = [pkg.SimClustersANNConfig(maxNumResults=c.maxNumResults, minScore=c.minScore, maxTopTweetsPerCluster=c.maxTopTweetsPerCluster,
                                   maxScanClusters=c.maxScanClusters, maxTweetCandidateAgeHours=c.maxTweetCandidateAgeHours,
                                   annAlgorithm=pkg.ScoringAlgorithm(alg)) for c in cfgs]
    return pkg.QueryBatch(index, d.emb_offsets, d.emb_cids, d.emb_scs, pc, now_ms=sd.NOW_MS)


def _same(ids, scores, counts, msz, q, o_ids, o_sc, o_msz, tag):
    assert counts[q] == len(o_ids), (tag, q, counts[q], len(o_ids))
    assert msz[q] == o_msz, (tag, q, msz[q], o_msz)
    assert np.array_equal(ids[q, :counts[q]], o_ids), (tag, q, "id order differs")
    assert np.array_equal(scores[q, :counts[q]].view(np.int64), np.asarray(o_sc).view(np.int64)), (tag, q, "scores differ")


# ---------------------------------------------------------------------------------------------------------------------
# descriptor kernel
M_CACHED = (M_ALL, 30, 5000, 100)  # the first four distinct M of a batch, in query order: cut tables
M_SEARCH = 7                        # the fifth: no table; inside the lists of 20, 45 and 200
LENGTHS = (0, 1, 3, 20, 45, 200)    # (0, 1, 3: shorter than P = 4; 20: shorter than M = 30; 45, 200: longer)

DESC_CASES = [
    # (P, clusters scanned per query (the last query is added: it scans the last row), last row's last partition non-empty)
    (32, (0, 1, 8, 9, 64, 50, 7, 33), True),     # rows of 64: 0, 32, 256, 288 and 2048 items (all eight slots full)
    (32, (0, 1, 8, 9, 64, 50, 7, 33), False),
    (32, (0, 1, 8, 9, 64, 65, 128, 33), True),   # rows of 128: 2080 items (the second group's first), 4096 (both groups full)
    (16, (0, 1, 16, 18, 64, 50, 7, 33), False),  # 0, 16, 256, 288 items
    (16, (0, 1, 16, 18, 64, 65, 128, 33), True),  # 1040 and 2048 items
    (4, (0, 1, 7, 64, 65, 128, 3, 50), True),    # one wave per query
    (8, (0, 1, 7, 64, 65, 128, 3, 50), False),
]


def _desc_design(lib, P, n_scans, last_nonempty):
    rng = np.random.default_rng([P, len(n_scans), int(last_nonempty), max(n_scans)])
    st = sd.streams(lib, P)
    pool = sd.id_pool()
    n_cl = max(n_scans) + 37
    lists, at = {}, 0
    for c in range(n_cl):
        n = LENGTHS[c % len(LENGTHS)]
        ids = pool[at:at + n].copy()
        at += n
        if n >= 20:  # a few tweets sit in the next long list too
            ids[:2] = pool[at:at + 2]
        lists[10 + c] = (ids, np.exp(rng.normal(-2.0, 1.0, n)))
    # the last row: three tweets, of partitions 0, 1 and -- or not -- P - 1
    parts = [0, 1 % P] + ([P - 1] if last_nonempty else [])
    last_ids = np.array([st[p][-1 - i] for i, p in enumerate(parts)], np.int64)
    last_cid = 10 + n_cl
    lists[last_cid] = (last_ids, np.exp(rng.normal(-2.0, 1.0, len(last_ids))))
    queries, embs = [], []
    for q, n in enumerate(tuple(n_scans) + (5,)):
        last = q == len(n_scans)
        M = M_SEARCH if q >= len(n_scans) - 1 else M_CACHED[q % 4]
        cl = 10 + rng.choice(n_cl, n, replace=False)
        if last:
            cl[-1] = last_cid
        embs.append((cl, np.exp(rng.normal(0.0, 0.5, n))))
        queries.append(sd.Query("desc", n, M, None))
    d = _design(P, queries, lists, embs)
    assert d.cluster_ids[-1] == last_cid
    lp = sd.partitions(lib, d.tweet_ids[d.list_offsets[-2]:], P)
    assert (int((lp == P - 1).sum()) > 0) == last_nonempty
    return d


@pytest.mark.parametrize("case", DESC_CASES, ids=lambda c: f"P{c[0]}-ns{max(c[1])}-last{'full' if c[2] else 'empty'}")
def test_descriptor_slots(pkg, oracle, lib, case):
    P, n_scans, last_nonempty = case
    d = _desc_design(lib, P, n_scans, last_nonempty)
    assert len(d.tweet_ids) < 300_000 and d.nq <= 64
    print(f"P = {P}: items per query {[Q.n_scan * P for Q in d.queries]}, M {[Q.M for Q in d.queries]}")
    T = sd.unit_T(lib, d)
    index = pkg.ClusterTweetIndex(d.cluster_ids, d.list_offsets, d.tweet_ids, d.scores, n_partitions=P)
    for alg in (2, 3):  # Cosine (the cluster-level cut's sort and sums), LogCosine
        tag = (P, max(n_scans), last_nonempty, alg)
        cfgs = [sd.Cfg(sd.K_FAST, Q.M, 24, alg) for Q in d.queries]
        qb = _batch(pkg, d, index, cfgs, alg)
        qb.run()
        uT = qb.unit_arrays()[0]
        assert np.array_equal(uT, T), (tag, "unit_T", np.argwhere(uT != T)[:8].tolist())
        qb.finish()
        ids, scores, counts, msz = qb.results()
        qb.close()
        for q in range(d.nq):
            cl, w = d.emb(q)
            o = oracle.sann_query(cl, w, None, cfgs[q], sd.NOW_MS, d.cluster_ids, d.list_offsets, d.tweet_ids, d.scores)
            _same(ids, scores, counts, msz, q, *o, tag)
    index.close()


# ---------------------------------------------------------------------------------------------------------------------
# merge staging
N_SCAN = 40
N_DUP = 2  # tweets per unit that sit in two of the query's clusters


def keep_all(k, P):
    """Live tweets up to which a unit offers all of them (sann_fast.hip; the launch may only raise it)."""
    kl = sd.unit_kl(k, P)
    return min(sd.FAST_SCAP, kl + kl // 2 + 16)


def _merge_design(lib, P, targets, windowed, seed):
    """Query q: targets[q] distinct tweets inside the window, spread evenly over the P units, N_DUP per unit in two
    clusters; a quarter as many again outside the window."""
    rng = np.random.default_rng([P, len(targets), int(windowed), seed])
    st = sd.streams(lib, P)
    lo, _hi = sd.window(WINDOW_H)
    inside = [s[s >= lo] if windowed else s for s in st]
    outside = [s[s < lo] if windowed else s[:0] for s in st]
    cur_in, cur_out = np.zeros(P, np.int64), np.zeros(P, np.int64)
    lists, queries, embs = {}, [], []
    for q, N in enumerate(targets):
        n_scan = min(N_SCAN, max(2, N))
        per = [[] for _ in range(n_scan)]
        for p in range(P):
            n_in, n_out = int(sd._split(N, P, q)[p]), int(sd._split(N // 4, P, q + 1)[p]) if windowed else 0
            a = inside[p][cur_in[p]:cur_in[p] + n_in]
            b = outside[p][cur_out[p]:cur_out[p] + n_out]
            assert len(a) == n_in and len(b) == n_out, "the id pool is too small for this design"
            cur_in[p] += n_in
            cur_out[p] += n_out
            for j, t in enumerate(a.tolist()):
                per[(j + p) % n_scan].append(t)
                if j < N_DUP:
                    per[(j + p + 1) % n_scan].append(t)
            for j, t in enumerate(b.tolist()):
                per[(j + p + 3) % n_scan].append(t)
        cl = 1000 * q + 1 + np.arange(n_scan)
        for c in range(n_scan):
            lists[int(cl[c])] = (np.array(per[c], np.int64), np.exp(rng.normal(-2.0, 1.0, len(per[c]))))
        embs.append((cl, np.exp(rng.normal(0.0, 0.5, n_scan))))
        queries.append(sd.Query("merge", n_scan, M_ALL, None))
    d = _design(P, queries, lists, embs)
    assert len(np.unique(d.scores)) == len(d.scores), "scores must be distinct"
    return d


MERGE_CASES = [
    # (P, k, distinct tweets inside the window per query) -> the merge kernels of launch_merge
    (32, 448, (200, 256, 257, 1024, 1025, 1800, 2100, 513, 1)),   # merge_kernel<512, 1728>: seven slots, 4 + 3
    (32, 1000, (200, 256, 257, 1024, 1025, 1800, 2100, 513, 1)),  # merge_kernel<1024, 2048>: eight slots, 4 + 4
    (8, 256, (100, 256, 257, 512, 513, 641, 800, 30, 1)),         # merge_wave_kernel<8, 16> up to 512, merge_kernel<256, 640> above
    (4, 128, (60, 255, 256, 257, 400, 3, 129, 128, 1)),           # merge_wave_kernel<4, 8> up to 256, merge_kernel<256, 640> above
]


@pytest.mark.parametrize("case", MERGE_CASES, ids=lambda c: f"P{c[0]}-k{c[1]}")
def test_merge_staging_slots(pkg, oracle, lib, case):
    P, k, targets = case
    d = _merge_design(lib, P, targets, True, 0)
    assert len(d.tweet_ids) < 300_000 and d.nq <= 64
    live = sd.unit_live(lib, d, WINDOW_H)
    assert live.sum(axis=1).tolist() == list(targets)
    assert live.max() <= keep_all(k, P), (int(live.max()), keep_all(k, P))  # every unit offers all it has
    index = pkg.ClusterTweetIndex(d.cluster_ids, d.list_offsets, d.tweet_ids, d.scores, n_partitions=P)
    for alg in (1, 3, 2):  # DotProduct, LogCosine, Cosine
        tag = (P, k, alg)
        free = [sd.Cfg(1000, M_ALL, WINDOW_H, alg) for _ in d.queries]
        cfgs = []
        for q in range(d.nq):  # a minScore that about half of the query's best thousand miss
            cl, w = d.emb(q)
            sc = oracle.sann_query(cl, w, None, free[q], sd.NOW_MS, d.cluster_ids, d.list_offsets, d.tweet_ids, d.scores)[1]
            assert len(sc) == min(targets[q], 1000) and sc[len(sc) // 2] > 0.0
            cfgs.append(sd.Cfg(k, M_ALL, WINDOW_H, alg, minScore=float(sc[len(sc) // 2])))
        qb = _batch(pkg, d, index, cfgs, alg)
        qb.run()
        _T, uniq, cnt, flags = qb.unit_arrays()
        staged = cnt.sum(axis=1).tolist()
        print(f"P = {P}, k = {k}, alg = {alg}: staged per query {staged}")
        assert staged == list(targets), (tag, staged)  # each query lands on the slot boundary it was built for
        assert np.array_equal(uniq, live), (tag, "unit_unique")
        assert not (flags & sd.UNIT_OVERFLOW).any(), tag
        qb.finish()
        ids, scores, counts, msz = qb.results()
        st = qb.stats()
        qb.close()
        for q in range(d.nq):
            cl, w = d.emb(q)
            o = oracle.sann_query(cl, w, None, cfgs[q], sd.NOW_MS, d.cluster_ids, d.list_offsets, d.tweet_ids, d.scores)
            _same(ids, scores, counts, msz, q, *o, tag)
            assert 0 < counts[q] < targets[q] or targets[q] == 1, (tag, q, counts[q])  # minScore dropped some, kept some
        assert st.n_requeried == 0 and st.n_fallback_units == 0, (tag, st.n_requeried, st.n_fallback_units)
    index.close()


def test_merge_staging_offline_norms(pkg, oracle, lib):
    """The offline forms: every staged entry's normaliser is the norms column (one more grouped trip)."""
    P, k, targets = 32, 448, (300, 600, 1025, 257, 1, 40, 256, 1024, 90)
    d = _merge_design(lib, P, targets, False, 1)
    d.norms = sd.full_norms(d)
    assert (d.norms > 0.0).all()
    live = sd.unit_live(lib, d, offline=True)
    assert live.sum(axis=1).tolist() == list(targets) and live.max() <= keep_all(k, P)
    rows = sd.sql_rows(oracle, d)
    index = pkg.ClusterTweetIndex(d.cluster_ids, d.list_offsets, d.tweet_ids, d.scores, n_partitions=P, tweet_norms=d.norms)
    for alg in (5, 6):
        tag = ("offline", alg)
        cfgs = [sd.Cfg(k, M_ALL, 175200, alg, minScore=-1e300) for _ in d.queries]
        qb = _batch(pkg, d, index, cfgs, alg)
        qb.run()
        staged = qb.unit_arrays()[2].sum(axis=1).tolist()
        assert staged == list(targets), (tag, staged)
        qb.finish()
        ids, scores, counts, msz = qb.results()
        st = qb.stats()
        qb.close()
        col = 3 if alg == 5 else 2
        for q in range(d.nq):
            want = sorted(rows[q], key=lambda r: (-r[col], r[0]))[:k]
            _same(ids, scores, counts, msz, q, np.array([r[0] for r in want], np.int64), np.array([r[col] for r in want]),
                  len(rows[q]), tag)
        assert st.n_requeried == 0 and st.n_fallback_units == 0, (tag, st.n_requeried, st.n_fallback_units)
    index.close()
