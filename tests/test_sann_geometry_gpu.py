"""Every production instantiation of unit_fast_kernel (8 geometries x 2 descriptor strides x NORMS) and the three
descriptor kernels, on designed corpora (tests/_sann_design.py) that put units at the edges of each geometry:
T == WG*U, one posting more, the match list's path thresholds, 64 / 65 / 128 / 129 scanned clusters, cached cut
tables and (the last query of every batch: an M inside its sub-lists that no table is cached for) the binary search.

Bit-equality with the oracle alone would also pass if a broken instantiation overflowed or got its queries re-run
every time (both re-runs are exact).  So, between run() and finish(), the per-unit arrays are compared with the host
model, and afterwards `n_requeried == 0` and `n_fallback_units ==` the designed overflows: the fast path's own answer
is what gets compared.  tests/test_sann_design_cpu.py shows that the designs alone meet those two conditions."""
import numpy as np
import pytest

import _sann_design as sd

pytestmark = pytest.mark.gpu

ONLINE_ALGS = (1, 2, 3, 4)   # DotProduct, Cosine, LogCosine, the no-source-norm form
OFFLINE_ALGS = (5, 6)        # OfflineLogCosine, OfflineCosine


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def _batch(pkg, d, index, cfgs, sources, alg):
    pc = [pkg.SimClustersANNConfig(maxNumResults=c.maxNumResults, minScore=c.minScore, maxTopTweetsPerCluster=c.maxTopTweetsPerCluster,
                                   maxScanClusters=c.maxScanClusters, maxTweetCandidateAgeHours=c.maxTweetCandidateAgeHours,
                                   annAlgorithm=pkg.ScoringAlgorithm(alg)) for c in cfgs]
    src = np.array([0 if s is None else s for s in sources], np.int64)
    has = np.array([0 if s is None else 1 for s in sources], np.uint8)
    return pkg.QueryBatch(index, d.emb_offsets, d.emb_cids, d.emb_scs, pc, now_ms=sd.NOW_MS, source_tweet_ids=src, has_source_tweet=has)


def _check_units(lib, d, qb, T, live, designed, tag):
    """After run(), before finish(): the descriptor kernels' counts, the overflow flags and the unit kernel's count of
    distinct tweets, unit by unit."""
    uT, uniq, cnt, flags = qb.unit_arrays()
    reasons = qb.overflow_reasons()
    narrow = np.array([Q.n_scan <= sd.NSCAN_MAX for Q in d.queries])
    assert np.array_equal(uT[narrow], T[narrow]), (tag, "unit_T", np.argwhere(uT != T)[:8].tolist())
    over = (flags & sd.UNIT_OVERFLOW) != 0
    assert np.array_equal(over, designed != 0), (tag, "overflow flags", np.argwhere(over != (designed != 0))[:8].tolist(), reasons.tolist())
    assert reasons.tolist() == [0] + [int((designed == r).sum()) for r in range(1, 8)], (tag, "overflow reasons", reasons.tolist())
    ok = ~over
    assert np.array_equal(uniq[ok], live[ok]), (tag, "unit_unique", np.argwhere((uniq != live) & ok)[:8].tolist())
    assert cnt.max() <= sd.FAST_SCAP, (tag, "cand_cnt", int(cnt.max()))
    return int(over.sum())


def _same(ids, scores, counts, msz, q, o_ids, o_sc, o_msz, tag):
    assert counts[q] == len(o_ids), (tag, q, counts[q], len(o_ids))
    assert msz[q] == o_msz, (tag, q, msz[q], o_msz)
    assert np.array_equal(ids[q, :counts[q]], o_ids), (tag, q, "id order differs")
    assert np.array_equal(scores[q, :counts[q]].view(np.int64), np.asarray(o_sc).view(np.int64)), (tag, q, "scores differ")


@pytest.mark.parametrize("case", sd.online_cases(), ids=sd.case_id)
def test_geometry_online(pkg, oracle, lib, monkeypatch, case):
    cap, wide, P = case
    monkeypatch.setenv("SANN_UNIT_CAP", str(cap))  # read when a batch is prepared; wins over the a-priori bound and the hint
    d = sd.design(lib, case)
    WG, U = sd.GEOMETRY[cap]
    print(f"unit_fast_kernel<{WG}, {U}, {128 if wide else 64}, 0, false>, P = {P}, nq = {d.nq}")
    T = sd.unit_T(lib, d)
    index = pkg.ClusterTweetIndex(d.cluster_ids, d.list_offsets, d.tweet_ids, d.scores, n_partitions=P)
    for name in sd.CONFIGURATIONS:
        fast = name != "k1000"
        if fast:
            _c, sources, hours = sd.configuration(d, name, 1)
            live = sd.unit_live(lib, d, hours, sources)
            designed = sd.designed_overflows(lib, d, T, hours, sources)
        for alg in ONLINE_ALGS:
            tag = (sd.case_id(case), name, alg)
            cfgs, sources, _h = sd.configuration(d, name, alg)
            qb = _batch(pkg, d, index, cfgs, sources, alg)
            qb.run()
            n_over = _check_units(lib, d, qb, T, live, designed, tag) if fast else None
            qb.finish()
            ids, scores, counts, msz = qb.results()
            st = qb.stats()
            qb.close()
            for q in range(d.nq):
                cl, w = d.emb(q)
                o = oracle.sann_query(cl, w, sources[q], cfgs[q], sd.NOW_MS, d.cluster_ids, d.list_offsets, d.tweet_ids, d.scores)
                _same(ids, scores, counts, msz, q, *o, tag)
            if fast:  # the slow path hid nothing: no query was re-run, and only the designed overflows fell back
                assert st.n_requeried == 0, (tag, st.n_requeried)
                assert st.n_fallback_units == n_over, (tag, st.n_fallback_units, n_over)
    index.close()


@pytest.mark.parametrize("case", sd.offline_cases(), ids=sd.case_id)
def test_geometry_offline(pkg, oracle, lib, monkeypatch, case):
    """The NORMS instantiations: the two offline forms on an index built with tweet_norms, against the restated SQL.
    (The job has no age window and no source tweet: the configurations are k = 24 and k = 1000.  The SQL orders by the
    log-cosine column; the cosine form's expected answer is the same rows ordered by their cosine column.)"""
    cap, wide, P = case
    monkeypatch.setenv("SANN_UNIT_CAP", str(cap))
    d = sd.design(lib, case, offline=True)
    WG, U = sd.GEOMETRY[cap]
    print(f"unit_fast_kernel<{WG}, {U}, {128 if wide else 64}, 0, true>, P = {P}, nq = {d.nq}")
    T = sd.unit_T(lib, d)
    live = sd.unit_live(lib, d, offline=True)
    none = [None] * d.nq
    designed = sd.designed_overflows(lib, d, T, 0, none, offline=True)
    rows = sd.sql_rows(oracle, d)  # per query: (tweet, dot, cosine, log-cosine), every row of the job
    index = pkg.ClusterTweetIndex(d.cluster_ids, d.list_offsets, d.tweet_ids, d.scores, n_partitions=P, tweet_norms=d.norms)
    for k in (sd.K_FAST, 1000):
        fast = k == sd.K_FAST
        for alg in OFFLINE_ALGS:
            tag = (sd.case_id(case), "offline", k, alg)
            cfgs = [sd.Cfg(k, Q.M, 175200, alg, minScore=-1e300) for Q in d.queries]
            qb = _batch(pkg, d, index, cfgs, none, alg)
            qb.run()
            n_over = _check_units(lib, d, qb, T, live, designed, tag) if fast else None
            qb.finish()
            ids, scores, counts, msz = qb.results()
            st = qb.stats()
            qb.close()
            col = 3 if alg == 5 else 2
            for q in range(d.nq):
                want = sorted(rows[q], key=lambda r: (-r[col], r[0]))[:k]
                # (the map's size: the number of rows the job has for the user)
                _same(ids, scores, counts, msz, q, np.array([r[0] for r in want], np.int64), np.array([r[col] for r in want]),
                      len(rows[q]), tag)
            if fast:
                assert st.n_requeried == 0, (tag, st.n_requeried)
                assert st.n_fallback_units == n_over, (tag, st.n_fallback_units, n_over)
    index.close()
