"""The merge kernels after their issue-slot cuts (profiles/NOTES.md, round 13): the one-compare 128-bit wave sort, the final
sort padded with pairwise distinct keys (no tie rule in the merge rounds), and staged entries addressed through one LDS
word per unit.  Every query of every case is compared with the oracle bit for bit: ids, score bits, count, map size.

Cosine with single-cluster candidates.  A tweet met in one cluster scores w * s / sqrt(s * s): the cluster's weight, to the
last few ulps -- exactly w where s is a power of two, as it is in every other cluster here.  Whole clusters tie on the
score key and the id key decides, in the wave sort, in the merge rounds and at the cut.  A unit that has no more live
tweets than `keep_all` offers all of them, so with the largest k of a case a query stages exactly as many entries as it
has tweets inside the window: the designs put that number on both sides of 64 (one run), 128, 256, 512 (the runs of the
final sort, merge_wave_kernel's capacity) and of MERGE_LDS (a second tournament round), at a query with fewer than k
candidates and at one with none, and the test asserts it from cand_cnt.  The smaller k of a case run on the same index
(units then withhold, and the proof decides).  P = 32 runs merge_kernel<512, 1728> and <1024, 2048>; P = 8, 4 and 1
run merge_wave_kernel<8, 16> / <4, 8> for the small queries and merge_kernel<256, 640> for the others.

The duplicate-heavy corpus is the 1M-tweet benchmark corpus at test size: every unit meets tweets it has already seen and
settles them through the sorted match list, the unit kernel's use of the same wave sort."""
import numpy as np
import pytest

import _sann_design as sd

pytestmark = pytest.mark.gpu

M_ALL = 20000
WINDOW_H = 12
COSINE = 2
N_SCAN = 6


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def keep_all(k, P):
    """Live tweets up to which a unit offers all of them (sann_fast.hip; the launch may only raise it)."""
    kl = sd.unit_kl(k, P)
    return min(sd.FAST_SCAP, kl + kl // 2 + 16)


def _design(lib, P, targets):
    """Query q: targets[q] tweets inside the window, each in ONE of the query's clusters, spread evenly over the P units; a
    quarter as many again (at least 8) outside the window.  Even clusters carry power-of-two scores."""
    rng = np.random.default_rng([13, P, len(targets)])
    st = sd.streams(lib, P)
    lo, _hi = sd.window(WINDOW_H)
    inside, outside = [s[s >= lo] for s in st], [s[s < lo] for s in st]
    cur_in, cur_out = np.zeros(P, np.int64), np.zeros(P, np.int64)
    cids, offs, tid, sc, embs, queries = [], [0], [], [], [], []
    for q, N in enumerate(targets):
        per = [[] for _ in range(N_SCAN)]
        for p in range(P):
            n_in, n_out = int(sd._split(N, P, q)[p]), int(sd._split(max(8, N // 4), P, q + 1)[p])
            a, b = inside[p][cur_in[p]:cur_in[p] + n_in], outside[p][cur_out[p]:cur_out[p] + n_out]
            assert len(a) == n_in and len(b) == n_out, "the id pool is too small for this design"
            cur_in[p] += n_in
            cur_out[p] += n_out
            for j, t in enumerate(a.tolist() + b.tolist()):
                per[(j + p) % N_SCAN].append(t)
        cl = 1000 * q + 1 + np.arange(N_SCAN)
        for c in range(N_SCAN):
            ids = np.array(per[c], np.int64)
            s = 2.0 ** -rng.integers(1, 4, len(ids)) if c % 2 == 0 else np.exp(rng.normal(-2.0, 1.0, len(ids)))
            order = np.lexsort((ids, -s))  # the store's order: score descending, id ascending
            cids.append(int(cl[c])), tid.append(ids[order]), sc.append(s[order]), offs.append(offs[-1] + len(ids))
        embs.append((cl, np.exp(rng.normal(0.0, 0.5, N_SCAN))))
        queries.append(sd.Query("merge", N_SCAN, M_ALL, None))
    eo = np.arange(len(targets) + 1, dtype=np.int64) * N_SCAN
    return sd.Design(0, P, False, queries, np.array(cids, np.int32), np.array(offs, np.int64), np.concatenate(tid), np.concatenate(sc),
                     eo, np.concatenate([e[0] for e in embs]).astype(np.int32), np.concatenate([e[1] for e in embs]))


def _same(ids, scores, counts, msz, q, o_ids, o_sc, o_msz, tag):
    assert counts[q] == len(o_ids), (tag, q, counts[q], len(o_ids))
    assert msz[q] == o_msz, (tag, q, msz[q], o_msz)
    assert np.array_equal(ids[q, :counts[q]], o_ids), (tag, q, "id order differs")
    assert np.array_equal(scores[q, :counts[q]].view(np.int64), np.asarray(o_sc).view(np.int64)), (tag, q, "scores differ")


def _run(pkg, oracle, d, index, k, tag):
    """-> (staged entries per query, batch stats, oracle answers); every query compared with the oracle"""
    cfgs = [sd.Cfg(k, M_ALL, WINDOW_H, COSINE) for _ in d.queries]
    pc = [pkg.SimClustersANNConfig(maxNumResults=c.maxNumResults, minScore=c.minScore, maxTopTweetsPerCluster=c.maxTopTweetsPerCluster,
                                   maxScanClusters=c.maxScanClusters, maxTweetCandidateAgeHours=c.maxTweetCandidateAgeHours,
                                   annAlgorithm=pkg.ScoringAlgorithm(COSINE)) for c in cfgs]
    qb = pkg.QueryBatch(index, d.emb_offsets, d.emb_cids, d.emb_scs, pc, now_ms=sd.NOW_MS)
    qb.run()
    _T, _uniq, cnt, flags = qb.unit_arrays()
    qb.finish()
    ids, scores, counts, msz = qb.results()
    st = qb.stats()
    qb.close()
    answers = []
    for q in range(d.nq):
        cl, w = d.emb(q)
        o = oracle.sann_query(cl, w, None, cfgs[q], sd.NOW_MS, d.cluster_ids, d.list_offsets, d.tweet_ids, d.scores)
        _same(ids, scores, counts, msz, q, *o, tag)
        answers.append(o)
    return cnt.sum(axis=1).tolist(), flags, st, answers


CASES = [
    # (P, k values (the last is the largest: with it every unit offers all it has), MERGE_LDS of the workgroup kernel,
    #  tweets inside the window per query)
    (32, (1, 63, 64, 65, 128, 256, 400, 448), 1728, (64, 65, 128, 129, 256, 257, 512, 513, 1728, 1729, 40, 0)),
    (32, (449, 1000), 2048, (64, 65, 128, 129, 256, 257, 512, 513, 2048, 2049, 40, 0)),
    (8, (1, 63, 64, 65, 128, 256), 640, (64, 65, 128, 129, 256, 257, 512, 513, 640, 641, 40, 0)),
    (4, (1, 63, 64, 65, 128), 640, (64, 65, 128, 129, 256, 257, 400, 40, 0)),  # (four units hold 448 at the most)
    (1, (1, 63, 64, 65, 128), 640, (64, 65, 128, 129, 160, 40, 0)),            # (one unit holds 160)
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"P{c[0]}-kmax{c[1][-1]}")
def test_cosine_ties_decided_by_id(pkg, oracle, lib, case):
    P, ks, merge_lds, targets = case
    d = _design(lib, P, targets)
    assert len(d.tweet_ids) < 300_000 and d.nq <= 64
    live = sd.unit_live(lib, d, WINDOW_H)
    assert live.sum(axis=1).tolist() == list(targets)
    assert live.max() <= keep_all(ks[-1], P), (int(live.max()), keep_all(ks[-1], P))
    index = pkg.ClusterTweetIndex(d.cluster_ids, d.list_offsets, d.tweet_ids, d.scores, n_partitions=P)
    try:
        for k in ks:
            staged, flags, st, answers = _run(pkg, oracle, d, index, k, (P, k))
            print(f"P = {P}, k = {k}: staged per query {staged}, re-answered {st.n_requeried}")
            assert not (flags & sd.UNIT_OVERFLOW).any() and st.n_fallback_units == 0, (P, k)
            if k != ks[-1]:
                continue
            assert staged == list(targets), (P, k, staged)  # each query lands on the boundary it was built for
            assert st.n_requeried == 0, (P, k, st.n_requeried)
            for edge in (64, 128, 256, 512, merge_lds):
                if edge < max(targets):
                    assert edge in staged and edge + 1 in staged, (P, edge, staged)
            assert 0 in staged and any(0 < s < k for s in staged)  # a query without candidates, one with fewer than k
            for q, (o_ids, o_sc, _m) in enumerate(answers):  # the regime: far fewer distinct scores than answers
                if len(o_ids) >= 64:
                    assert len(np.unique(o_sc)) <= len(o_sc) // 4, (P, q, len(np.unique(o_sc)), len(o_sc))
    finally:
        index.close()


DUP_P = 8


def test_duplicate_heavy_corpus_sorted_settle(pkg, oracle, lib):
    """50 k tweets in one to three of 800 clusters, a query scans 50 of the popular ones: every unit meets 20 ... 90 postings
    of tweets it has already seen, and units with 13 ... 64 of them settle through the sorted match list."""
    co = pkg.corpus.make_corpus(50000, 800, seed=131, index_cap=300, mean_clusters=1.2, max_clusters_per_tweet=3)
    offs, cids, scs = pkg.corpus.make_queries(24, 800, seed=132, clusters_per_user=50)
    nq = len(offs) - 1
    dup = np.zeros((nq, DUP_P), np.int64)
    for q in range(nq):
        ids = np.concatenate([co.list_of(int(c))[0] for c in cids[offs[q]:offs[q + 1]]])
        part = sd.partitions(lib, ids, DUP_P)
        for p in range(DUP_P):
            _u, inv, n_occ = np.unique(ids[part == p], return_inverse=True, return_counts=True)
            dup[q, p] = int((n_occ[inv] > 1).sum())
    sorted_path = (dup >= 16) & (dup <= 56)  # (Bloom collisions may add a few entries: this stays inside 13 ... 64)
    assert sorted_path.sum() >= 48, np.sort(dup.reshape(-1)).tolist()
    index = pkg.ClusterTweetIndex(co.cluster_ids, co.list_offsets, co.tweet_ids, co.scores, n_partitions=DUP_P)
    try:
        for alg in (2, 3):  # Cosine, LogCosine
            cfgs = [pkg.SimClustersANNConfig(maxNumResults=100, maxTopTweetsPerCluster=300, maxScanClusters=50,
                                             annAlgorithm=pkg.ScoringAlgorithm(alg)) for _ in range(nq)]
            qb = pkg.QueryBatch(index, offs, cids, scs, cfgs, now_ms=co.now_ms)
            qb.run()
            flags = qb.unit_arrays()[3]
            qb.finish()
            ids, scores, counts, msz = qb.results()
            qb.close()
            assert (((flags & sd.UNIT_OVERFLOW) == 0) & sorted_path).sum() >= 48, "units of the sorted path stayed on the fast path"
            for q in range(nq):
                o = oracle.sann_query(cids[offs[q]:offs[q + 1]], scs[offs[q]:offs[q + 1]], None, cfgs[q], co.now_ms,
                                      co.cluster_ids, co.list_offsets, co.tweet_ids, co.scores)
                _same(ids, scores, counts, msz, q, *o, ("dup-heavy", alg))
    finally:
        index.close()
