"""The id column of a persistent index and the id form of unit_fast_kernel (cosine forms: phase 2 gathers the 8-byte
tweet ids of the column instead of the 16-byte postings).

1. the column holds the postings' ids, position by position, after each of the three persistent builders;
2. the id form, the same batch with SANN_ID_COLUMN=0 (the 16-byte form) and the oracle agree bit for bit -- ids, score
   bits, counts, map sizes -- at every unit geometry, both descriptor strides and P in {4, 32}, on designed corpora
   (tests/_sann_design.py) whose units sit at the edges of the gather; the edges are asserted from the device's own
   unit_T (sann_debug_unit_arrays) and from a host model of the index's sub-list offsets;
3. the age window and the source-tweet exclusion still see the id;
4. tweets in two and three scanned clusters (short match list), the 13 ... 64-entry sorted path, and a duplicate-heavy
   random corpus;
5. what must NOT take the id form: an index with a score outside (1e-15, 1e15), a batch mixing cosine and LogCosine
   configs, the offline cosine form on an index with norms, an index without the column.

Which path answered is read from sann_debug_id_column (QueryBatch.id_column): `used` is asserted in every run."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import _sann_design as sd

pytestmark = pytest.mark.gpu

K = 40
COSINE_ALGS = (2, 4)  # CosineSimilarity, the no-source-norm form


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


# ---------------------------------------------------------------------------------------------------------------------
# helpers
def _cfg(pkg, c):
    return pkg.SimClustersANNConfig(maxNumResults=c.maxNumResults, minScore=c.minScore, maxTopTweetsPerCluster=c.maxTopTweetsPerCluster,
                                    maxScanClusters=c.maxScanClusters, maxTweetCandidateAgeHours=c.maxTweetCandidateAgeHours,
                                    annAlgorithm=pkg.ScoringAlgorithm(c.annAlgorithm))


def _batch(pkg, index, emb, cfgs, sources, now_ms):
    offs, cids, scs = emb
    src = np.array([0 if s is None else s for s in sources], np.int64)
    has = np.array([0 if s is None else 1 for s in sources], np.uint8)
    return pkg.QueryBatch(index, offs, cids, scs, [_cfg(pkg, c) for c in cfgs], now_ms=now_ms, source_tweet_ids=src, has_source_tweet=has)


def _run(qb):
    """run(); the unit arrays and the path as the run left them; finish().  -> (results, unit arrays, id_column(), stats)."""
    qb.run()
    units = qb.unit_arrays()
    path = qb.id_column()
    qb.finish()
    return qb.results(), units, path, qb.stats()


def _bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same_runs(a, b, tag):
    """Two runs of one batch: counts and map sizes equal, and every row's ids and score bits up to its count (what lies
    behind a row's count is not part of the answer)."""
    assert np.array_equal(a[2], b[2]), (tag, "counts", np.argwhere(a[2] != b[2])[:4].tolist())
    assert np.array_equal(a[3], b[3]), (tag, "map sizes", np.argwhere(a[3] != b[3])[:4].tolist())
    for q, n in enumerate(a[2]):
        assert np.array_equal(a[0][q, :n], b[0][q, :n]), (tag, "ids", q)
        assert np.array_equal(_bits(a[1][q, :n]), _bits(b[1][q, :n])), (tag, "scores", q)


def _same_oracle(out, q, o_ids, o_sc, o_msz, tag):
    ids, scores, counts, msz = out
    assert counts[q] == len(o_ids), (tag, q, counts[q], len(o_ids))
    assert msz[q] == o_msz, (tag, q, msz[q], o_msz)
    assert np.array_equal(ids[q, :counts[q]], o_ids), (tag, q, "id order differs")
    assert np.array_equal(scores[q, :counts[q]].view(np.int64), np.asarray(o_sc).view(np.int64)), (tag, q, "scores differ")


def _three_ways(pkg, oracle, monkeypatch, index, csr, emb, cfgs, sources, now_ms, tag, expect_used=True):
    """The batch with the id form allowed and with SANN_ID_COLUMN=0, both against the oracle.  -> the first run's
    (results, unit arrays, stats)."""
    cluster_ids, list_offsets, tweet_ids, scores = csr
    offs, cids, scs = emb
    monkeypatch.delenv("SANN_ID_COLUMN", raising=False)
    qb = _batch(pkg, index, emb, cfgs, sources, now_ms)
    out, units, path, st = _run(qb)
    qb.close()
    assert path[2] == expect_used, (tag, "id form used", path)
    monkeypatch.setenv("SANN_ID_COLUMN", "0")
    qb = _batch(pkg, index, emb, cfgs, sources, now_ms)
    out16, _units16, path16, _st16 = _run(qb)
    qb.close()
    monkeypatch.delenv("SANN_ID_COLUMN", raising=False)
    assert not path16[2], (tag, "SANN_ID_COLUMN=0 must keep the 16-byte form", path16)
    _same_runs(out, out16, tag)
    for q in range(len(offs) - 1):
        o = oracle.sann_query(cids[offs[q]:offs[q + 1]], scs[offs[q]:offs[q + 1]], sources[q], cfgs[q], now_ms, cluster_ids, list_offsets,
                              tweet_ids, scores)
        _same_oracle(out, q, *o, tag)
    return out, units, st


def _csr(d):
    return d.cluster_ids, d.list_offsets, d.tweet_ids, d.scores


def _emb(d):
    return d.emb_offsets, d.emb_cids, d.emb_scs


# ---------------------------------------------------------------------------------------------------------------------
# 1. column = postings
def _check_column(index, clusters):
    n = 0
    for c in clusters:
        want = index.get_list(int(c))[0]
        got = index.id_column_list(int(c))
        assert np.array_equal(want, got), (int(c), len(want), len(got))
        n += len(want)
    return n


@pytest.fixture(scope="module")
def small(pkg):
    return pkg.corpus.make_corpus(20000, 800, seed=31, index_cap=300)


@pytest.mark.parametrize("n_shards", [1, 2])
def test_column_equals_postings(pkg, small, n_shards):
    co = small
    held = 0
    for shard in range(n_shards):
        kw = dict(n_partitions=8, shard_id=shard, n_shards=n_shards)
        built = [
            pkg.ClusterTweetIndex(co.cluster_ids, co.list_offsets, co.tweet_ids, co.scores, **kw),
            pkg.ClusterTweetIndex.from_raw_postings(co.cluster_ids, co.list_offsets, co.tweet_ids, co.scores, None, now_ms=co.now_ms,
                                                    max_results=300, **kw),
            pkg.ClusterTweetIndex.synthetic(20000, 800, index_cap=300, **kw),
        ]
        for i, index in enumerate(built):
            info = index.info()
            n = _check_column(index, index.cluster_ids)
            assert n == info.n_postings and n > 0, (i, n, info.n_postings)
            # postings 16 B, ranks 4 B, the column 8 B (padded to an even count), offsets
            assert info.device_bytes >= 28 * n and info.device_bytes - 28 * n <= 4 * (len(index.cluster_ids) * 8 + 1) + 32, (i, info.device_bytes, n)
            if i == 0:
                held += n
            index.close()
    assert held == len(co.tweet_ids)  # (the shards partition the corpus)


def test_column_of_an_index_without_postings(pkg):
    one = pkg.ClusterTweetIndex(np.array([7], np.int32), np.array([0, 0], np.int64), np.empty(0, np.int64), np.empty(0, np.float64), n_partitions=4)
    none = pkg.ClusterTweetIndex(np.empty(0, np.int32), np.array([0], np.int64), np.empty(0, np.int64), np.empty(0, np.float64), n_partitions=4)
    raw = pkg.ClusterTweetIndex.from_raw_postings(np.array([7], np.int32), np.array([0, 0], np.int64), np.empty(0, np.int64), np.empty(0, np.float64),
                                                  None, now_ms=sd.NOW_MS, n_partitions=4)
    for index in (one, none, raw):
        assert index.info().n_postings == 0
        assert len(index.id_column_list(7)) == 0  # (an error if the index had no column)
        cfg = pkg.SimClustersANNConfig(maxNumResults=K, annAlgorithm=pkg.ScoringAlgorithm(2))
        qb = pkg.QueryBatch(index, np.array([0, 1], np.int64), np.array([7], np.int32), np.array([1.0]), cfg, now_ms=sd.NOW_MS)
        out, _units, path, _st = _run(qb)
        qb.close()
        assert path[0] and path[1], path  # present; no score is out of range
        assert out[2][0] == 0
        index.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. same answer, bit for bit, at the edges of every geometry
def with_tail(lib, d):
    """The design plus one cluster, the index's LAST row, with three tweets in every partition, and one query that scans it
    alone: that query's unit of the last partition ends at the index's last posting."""
    st = sd.streams(lib, d.P)
    ids = np.concatenate([s[:3] for s in st])
    sc = 0.9 - 0.005 * np.arange(len(ids))
    cid = int(d.cluster_ids.max()) + 1
    return dataclasses.replace(
        d, queries=d.queries + [sd.Query("tail", 1, sd.M_ABOVE, None)], cluster_ids=np.append(d.cluster_ids, np.int32(cid)),
        list_offsets=np.append(d.list_offsets, d.list_offsets[-1] + len(ids)), tweet_ids=np.concatenate([d.tweet_ids, ids]),
        scores=np.concatenate([d.scores, sc]), emb_offsets=np.append(d.emb_offsets, d.emb_offsets[-1] + 1),
        emb_cids=np.append(d.emb_cids, np.int32(cid)), emb_scs=np.append(d.emb_scs, 1.0))


def sublists(lib, d):
    """Host model of the index layout (one shard): counts and start positions of every (row, partition) sub-list."""
    n_rows = len(d.cluster_ids)
    counts = np.zeros((n_rows, d.P), np.int64)
    for r in range(n_rows):
        a, b = int(d.list_offsets[r]), int(d.list_offsets[r + 1])
        if b > a:
            counts[r] = np.bincount(sd.partitions(lib, d.tweet_ids[a:b], d.P), minlength=d.P)
    starts = (np.cumsum(counts.reshape(-1)) - counts.reshape(-1)).reshape(n_rows, d.P)
    return counts, starts


def check_edges(lib, d, index, uT, flags, cap, tag):
    """The edges the gather can go wrong at are in this batch -- from the device's unit_T and the host model of the layout."""
    counts, starts = sublists(lib, d)
    n_postings = int(counts.sum())
    assert index.info().n_postings == n_postings, tag
    assert (uT == 0).any() and (uT == 1).any(), (tag, "T = 0 and T = 1")
    assert (uT == cap).any(), (tag, "T = WG * U exactly")
    over = uT == cap + 1
    assert over.any() and ((flags[over] & sd.UNIT_OVERFLOW) != 0).all(), (tag, "T one above the capacity overflows")
    assert (((uT % 64) != 0) & (uT > 64) & (uT <= cap)).any(), (tag, "T no multiple of 64")
    # row 0 is query 0's first cluster (ids ascend with the query): unit (0, 0) starts at position 0 of the index
    assert int(d.emb_cids[0]) == int(d.cluster_ids[0]) and counts[0, 0] > 0 and starts[0, 0] == 0 and uT[0, 0] > 0, tag
    # the tail query scans the last row whole: its unit of the last partition ends at n_postings - 1
    q = d.nq - 1
    assert int(d.emb_cids[-1]) == int(d.cluster_ids[-1]) and uT[q, d.P - 1] == counts[-1, d.P - 1] > 0, tag
    assert starts[-1, d.P - 1] + counts[-1, d.P - 1] == n_postings, tag
    assert ((starts % 2 == 1) & (counts > 0)).any(), (tag, "sub-lists that start at odd positions")


EDGE_CASES = [(cap, wide, P) for cap in sd.CAPS for wide in (False, True) for P in (4, 32)]


@pytest.mark.parametrize("case", EDGE_CASES, ids=sd.case_id)
def test_id_form_bit_for_bit(pkg, oracle, lib, monkeypatch, case):
    cap, wide, P = case
    monkeypatch.setenv("SANN_UNIT_CAP", str(cap))
    d = with_tail(lib, sd.design(lib, case))
    assert max(Q.n_scan for Q in d.queries if Q.n_scan <= sd.NSCAN_MAX) > 64 if wide else max(Q.n_scan for Q in d.queries) <= 64
    assert not wide or any(Q.n_scan == 65 for Q in d.queries)
    WG, U = sd.GEOMETRY[cap]
    print(f"unit_fast_kernel<{WG}, {U}, {128 if wide else 64}, 0, false, true>, P = {P}, nq = {d.nq}")
    index = pkg.ClusterTweetIndex(d.cluster_ids, d.list_offsets, d.tweet_ids, d.scores, n_partitions=P)
    none = [None] * d.nq
    for alg in COSINE_ALGS:
        tag = (sd.case_id(case), alg)
        cfgs = [sd.Cfg(K, Q.M, 24, alg) for Q in d.queries]
        _out, (uT, _uniq, cnt, flags), st = _three_ways(pkg, oracle, monkeypatch, index, _csr(d), _emb(d), cfgs, none, sd.NOW_MS, tag)
        check_edges(lib, d, index, uT, flags, cap, tag)
        assert cnt.max() <= sd.FAST_SCAP
        assert st.n_fallback_units == int(((flags & sd.UNIT_OVERFLOW) != 0).sum()), tag
    index.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. filters still see the id
@pytest.mark.parametrize("case", [(1536, False, 4), (1536, False, 32), (512, True, 4)], ids=sd.case_id)
def test_window_and_source_see_the_id(pkg, oracle, lib, monkeypatch, case):
    cap, _wide, P = case
    monkeypatch.setenv("SANN_UNIT_CAP", str(cap))
    d = sd.design(lib, case)
    index = pkg.ClusterTweetIndex(d.cluster_ids, d.list_offsets, d.tweet_ids, d.scores, n_partitions=P)
    sources = [Q.source for Q in d.queries]
    lo12, _hi = sd.window(12)
    n_src = 0
    for q, s in enumerate(sources):  # the source tweet is a posting of a cluster the query scans, inside the window
        if s is not None:
            ids = sd.scanned_postings(d, q)[0]
            assert s in ids
            n_src += int(s >= lo12)
    assert n_src >= 2
    scanned = np.concatenate([sd.scanned_postings(d, q)[0] for q in range(d.nq)])
    assert 0.2 < (scanned < lo12).mean() < 0.8, "the 12 h window cuts into the scanned lists"
    for alg in COSINE_ALGS:
        tag = (sd.case_id(case), alg)
        open_cfgs = [sd.Cfg(K, Q.M, 24, alg) for Q in d.queries]
        cfgs = [sd.Cfg(K, Q.M, 12, alg) for Q in d.queries]
        _o, (_t, uniq24, _c, _f), _s = _three_ways(pkg, oracle, monkeypatch, index, _csr(d), _emb(d), open_cfgs, [None] * d.nq, sd.NOW_MS, tag + ("open",))
        _o, (_t, uniq12, _c, flags), _s = _three_ways(pkg, oracle, monkeypatch, index, _csr(d), _emb(d), cfgs, sources, sd.NOW_MS, tag + ("12 h, source",))
        ok = (flags & sd.UNIT_OVERFLOW) == 0
        assert np.array_equal(uniq12[ok], sd.unit_live(lib, d, 12, sources)[ok]), (tag, "live tweets behind the filters")
        assert (uniq12[ok] < uniq24[ok]).any()
    index.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. duplicates
@pytest.mark.parametrize("case", [(1024, False, 8), (1536, False, 32)], ids=sd.case_id)
def test_duplicates_short_and_sorted_lists(pkg, oracle, lib, monkeypatch, case):
    """The designs' duplicates queries: tweets planted in two and in three scanned clusters of one unit; match lists of 12
    entries (settled by every wave for itself) and of 13 and 64 (sorted in registers)."""
    cap, _wide, P = case
    monkeypatch.setenv("SANN_UNIT_CAP", str(cap))
    d = sd.design(lib, case)
    nms = []
    for q, Q in enumerate(d.queries):
        if Q.role == "dup":
            nm, clean = sd.match_list(lib, d, q, Q.dup_unit)
            assert clean and nm == Q.nm, (q, nm, Q.nm)
            nms.append(nm)
            ids = sd.scanned_postings(d, q)[0]
            _u, n_occ = np.unique(ids, return_counts=True)
            assert (n_occ == 2).any() and (nm % 2 == 0 or (n_occ == 3).any()), (q, "tweets in two and in three clusters")
    assert {12, 13, 64} <= set(nms), nms
    index = pkg.ClusterTweetIndex(d.cluster_ids, d.list_offsets, d.tweet_ids, d.scores, n_partitions=P)
    for alg in COSINE_ALGS:
        cfgs = [sd.Cfg(K, Q.M, 24, alg) for Q in d.queries]
        _o, (_t, uniq, _c, flags), _s = _three_ways(pkg, oracle, monkeypatch, index, _csr(d), _emb(d), cfgs, [None] * d.nq, sd.NOW_MS, (sd.case_id(case), alg))
        ok = (flags & sd.UNIT_OVERFLOW) == 0
        assert np.array_equal(uniq[ok], sd.unit_live(lib, d)[ok]), "distinct live tweets per unit"
    index.close()


DUP_P = 8


@pytest.fixture(scope="module")
def dup_heavy(pkg, lib):
    """A small corpus under few clusters: 50 k tweets in one to three of 800 clusters, a query scans 50 of the popular ones,
    so every unit (800 ... 1200 postings) meets 20 ... 90 postings of tweets it has already seen.
    -> (corpus, queries, per unit: postings whose tweet occurs more than once in the unit)."""
    co = pkg.corpus.make_corpus(50000, 800, seed=41, index_cap=300, mean_clusters=1.2, max_clusters_per_tweet=3)
    offs, cids, scs = pkg.corpus.make_queries(32, 800, seed=42, clusters_per_user=50)
    dup = np.zeros((len(offs) - 1, DUP_P), np.int64)
    for q in range(len(offs) - 1):
        ids = np.concatenate([co.list_of(int(c))[0] for c in cids[offs[q]:offs[q + 1]]])
        part = sd.partitions(lib, ids, DUP_P)
        for p in range(DUP_P):
            _u, inv, n_occ = np.unique(ids[part == p], return_inverse=True, return_counts=True)
            dup[q, p] = int((n_occ[inv] > 1).sum())
    return co, (offs, cids, scs), dup


@pytest.mark.parametrize("cap", [1536, 4096])
def test_duplicate_heavy_corpus(pkg, oracle, monkeypatch, dup_heavy, cap):
    co, emb, dup = dup_heavy
    monkeypatch.setenv("SANN_UNIT_CAP", str(cap))
    # (every repeated posting is a match-list entry; Bloom collisions may add a few: 16 ... 56 stays inside 13 ... 64)
    assert ((dup >= 16) & (dup <= 56)).sum() >= 64, np.sort(dup.reshape(-1)).tolist()
    index = pkg.ClusterTweetIndex(co.cluster_ids, co.list_offsets, co.tweet_ids, co.scores, n_partitions=DUP_P)
    nq = len(emb[0]) - 1
    for alg in COSINE_ALGS:
        cfgs = [sd.Cfg(K, 300, 24, alg, maxScanClusters=50) for _ in range(nq)]
        _o, (uT, _u, _c, flags), _s = _three_ways(pkg, oracle, monkeypatch, index, (co.cluster_ids, co.list_offsets, co.tweet_ids, co.scores), emb,
                                                 cfgs, [None] * nq, co.now_ms, ("dup-heavy", cap, alg))
        fast = (flags & sd.UNIT_OVERFLOW) == 0
        assert uT.max() <= 1536
        assert (fast & (dup >= 16) & (dup <= 56)).sum() >= 64, "units of the sorted path stayed on the fast path"
    index.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. fallbacks: the 16-byte form answers, and answers right
def test_fallback_scores_out_of_range(pkg, oracle, monkeypatch, small):
    """One score of 1e20 and one of 1e-20 in scanned lists: the index's scores_ordinary is 0 and no batch takes the id form
    (the 16-byte form sends the units that meet those postings to the general path, as it always did)."""
    co = small
    offs, cids, scs = pkg.corpus.make_queries(32, 800, seed=32, clusters_per_user=50)
    scores = co.scores.copy()
    rows = [int(np.searchsorted(co.cluster_ids, c)) for c in cids[offs[0]:offs[1]] if len(co.list_of(int(c))[0]) > 4][:2]
    assert len(rows) == 2
    scores[co.list_offsets[rows[0]]] = 1e20           # a list's first (largest) score
    scores[co.list_offsets[rows[1] + 1] - 1] = 1e-20   # a list's last (smallest) score
    index = pkg.ClusterTweetIndex(co.cluster_ids, co.list_offsets, co.tweet_ids, scores, n_partitions=8)
    nq = len(offs) - 1
    for alg in COSINE_ALGS:
        cfgs = [sd.Cfg(K, 300, 24, alg, maxScanClusters=50) for _ in range(nq)]
        qb = _batch(pkg, index, (offs, cids, scs), cfgs, [None] * nq, co.now_ms)
        out, _units, path, _st = _run(qb)
        qb.close()
        assert path == (True, False, False), path
        for q in range(nq):
            o = oracle.sann_query(cids[offs[q]:offs[q + 1]], scs[offs[q]:offs[q + 1]], None, cfgs[q], co.now_ms, co.cluster_ids, co.list_offsets,
                                  co.tweet_ids, scores)
            _same_oracle(out, q, *o, ("out of range", alg))
    index.close()


def test_fallback_mixed_batch(pkg, oracle, small):
    co = small
    offs, cids, scs = pkg.corpus.make_queries(32, 800, seed=33, clusters_per_user=50)
    index = pkg.ClusterTweetIndex(co.cluster_ids, co.list_offsets, co.tweet_ids, co.scores, n_partitions=8)
    nq = len(offs) - 1
    cfgs = [sd.Cfg(K, 300, 24, 3 if q == nq // 2 else 2, maxScanClusters=50) for q in range(nq)]  # one LogCosine query among cosine ones
    qb = _batch(pkg, index, (offs, cids, scs), cfgs, [None] * nq, co.now_ms)
    out, _units, path, _st = _run(qb)
    assert path == (True, True, False), path
    for q in range(nq):
        o = oracle.sann_query(cids[offs[q]:offs[q + 1]], scs[offs[q]:offs[q + 1]], None, cfgs[q], co.now_ms, co.cluster_ids, co.list_offsets,
                              co.tweet_ids, co.scores)
        _same_oracle(out, q, *o, "mixed")
    # the same batch object, reset to cosine alone, takes the id form; reset to the mixed batch, it leaves it again
    pure = [_cfg(pkg, sd.Cfg(K, 300, 24, 2, maxScanClusters=50))] * nq
    qb.reset(offs, cids, scs, pure, now_ms=co.now_ms)
    assert _run(qb)[2] == (True, True, True)
    qb.reset(offs, cids, scs, [_cfg(pkg, c) for c in cfgs], now_ms=co.now_ms)
    out2, _units, path2, _st = _run(qb)
    assert path2 == (True, True, False)
    _same_runs(out, out2, "mixed, after a reset")
    qb.close()
    index.close()


def test_fallback_offline_cosine_on_norms(pkg, oracle, lib, monkeypatch):
    case = (1536, False, 8)
    monkeypatch.setenv("SANN_UNIT_CAP", "1536")
    d = sd.design(lib, case, offline=True)
    rows = sd.sql_rows(oracle, d)  # per query: (tweet, dot, cosine, log-cosine)
    index = pkg.ClusterTweetIndex(d.cluster_ids, d.list_offsets, d.tweet_ids, d.scores, n_partitions=8, tweet_norms=d.norms)
    cfgs = [sd.Cfg(sd.K_FAST, Q.M, 175200, 6, minScore=-1e300) for Q in d.queries]
    qb = _batch(pkg, index, _emb(d), cfgs, [None] * d.nq, sd.NOW_MS)
    out, _units, path, _st = _run(qb)
    qb.close()
    assert path[0] and not path[2], path
    for q in range(d.nq):
        want = sorted(rows[q], key=lambda r: (-r[2], r[0]))[:sd.K_FAST]
        _same_oracle(out, q, np.array([r[0] for r in want], np.int64), np.array([r[2] for r in want]), len(rows[q]), "offline cosine")
    index.close()


def test_fallback_index_without_the_column(pkg, oracle, lib, small):
    """The per-batch index of the cluster-range deployment (sann_index_build_from_device_postings) builds no column."""
    co = small
    sa = pkg.simclusters_ann
    offs, cids, scs = pkg.corpus.make_queries(32, 800, seed=34, clusters_per_user=50)
    post = np.zeros(len(co.tweet_ids), np.dtype([("id", np.int64), ("score", np.float64)]))
    post["id"], post["score"] = co.tweet_ids, co.scores
    d_post = C.c_void_p()
    assert lib.sann_device_alloc(0, max(post.nbytes, 16), C.byref(d_post)) == 0, lib.sann_last_error()
    assert lib.sann_device_copy(0, d_post, post.ctypes.data_as(C.c_void_p), post.nbytes) == 0, lib.sann_last_error()
    opts = sa.sann_index_options_t(0, 8, 0, 1)
    h = C.c_void_p()
    cl, lo = np.ascontiguousarray(co.cluster_ids, np.int32), np.ascontiguousarray(co.list_offsets, np.int64)
    rc = lib.sann_index_build_from_device_postings(C.byref(opts), len(cl), cl.ctypes.data_as(C.c_void_p), lo.ctypes.data_as(C.c_void_p), d_post, C.byref(h))
    assert rc == 0, lib.sann_last_error()
    index = sa.ClusterTweetIndex.__new__(sa.ClusterTweetIndex)
    index._h, index.device, index.cluster_ids, index.list_offsets = h, 0, cl, lo
    with pytest.raises(sa.SannError):
        index.id_column_list(int(cl[0]))
    nq = len(offs) - 1
    cfgs = [sd.Cfg(K, 300, 24, 2, maxScanClusters=50) for _ in range(nq)]
    qb = _batch(pkg, index, (offs, cids, scs), cfgs, [None] * nq, co.now_ms)
    out, _units, path, _st = _run(qb)
    qb.close()
    assert path == (False, False, False), path
    for q in range(nq):
        o = oracle.sann_query(cids[offs[q]:offs[q + 1]], scs[offs[q]:offs[q + 1]], None, cfgs[q], co.now_ms, co.cluster_ids, co.list_offsets,
                              co.tweet_ids, co.scores)
        _same_oracle(out, q, *o, "no column")
    index.close()
    assert lib.sann_device_free(0, d_post) == 0
