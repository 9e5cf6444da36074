"""The designed corpora of tests/_sann_design.py, checked against the oracle on the host: what the device sweep
(tests/test_sann_geometry_gpu.py) takes for granted about a design is shown here, from the design alone.  A design
that fails gets another seed in _sann_design.SEEDS; the assertions on the device stay as they are."""
import numpy as np
import pytest

import _sann_design as sd

ONLINE_ALGS = (1, 2, 3, 4)
CASES = [(c, False) for c in sd.online_cases()] + [(c, True) for c in sd.offline_cases()]


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def test_id_streams_are_the_library_partitions(lib):
    """The streams really are the library's partitions, at every P the sweep uses."""
    for P in (1, 2, 4, 8, 16, 32):
        st = sd.streams(lib, P)
        assert sum(len(s) for s in st) == len(sd.id_pool())
        for p in (0, P - 1):
            assert all(lib.sann_tweet_partition(int(t), P) == p for t in st[p][:200].tolist())
        assert min(len(s) for s in st) >= 4097 + 400  # (the largest unit, behind a reseeded design's offset)


def test_unit_kl_restated():
    """share + five sigma + 4, capped by k: the figures the unit kernel's header quotes."""
    assert sd.unit_kl(400, 32) == 34
    assert (sd.unit_kl(24, 1), sd.unit_kl(24, 8), sd.unit_kl(24, 32)) == (24, 15, 9)
    assert sd.unit_kl(1000, 1) == 128
    assert (sd.quota(24, 1), sd.quota(24, 8), sd.quota(24, 32)) == (24, 14, 8)


@pytest.mark.parametrize("case,offline", CASES, ids=[sd.case_id(c) + ("-offline" if o else "") for c, o in CASES])
def test_design(lib, oracle, case, offline):
    cap, wide, P = case
    d = sd.design(lib, case, offline)
    WG, U = sd.GEOMETRY[cap]
    assert WG * U == cap and d.nq % 8 == 1
    T = sd.unit_T(lib, d)
    roles = [Q.role for Q in d.queries]
    # ---- band: the designed unit sizes are what the model counts, and lie where the case claims
    for q, Q in enumerate(d.queries):
        if Q.sizes is not None and Q.role != "fill":
            assert np.array_equal(T[q], Q.sizes), (q, Q.role)
        if Q.band is not None:
            assert ((T[q] > Q.band[0]) & (T[q] <= Q.band[1])).all(), (q, Q.role, T[q])
    assert (T[roles.index("full")] == cap).all()
    over = T[roles.index("over")]
    assert (over > cap).sum() == 1 and over.max() == cap + 1 and ((over == cap - 1) | (over == cap + 1)).all()
    spread = np.concatenate([T[q] for q, r in enumerate(roles) if r == "spread"])
    want = {sd.prev_cap(cap) + 1, cap - WG + 1, cap - 1, cap}
    assert set(spread.tolist()) == want
    small = np.concatenate([T[q] for q, r in enumerate(roles) if r == "small"])
    if P >= 4:
        assert set(small.tolist()) == {0, 1, 63, 65}
    assert sorted(Q.n_scan for Q in d.queries if Q.role == "small") == [1, 50, 63, 64]
    assert (T[roles.index("m_zero")] == 0).all()
    mb = roles.index("m_below")
    assert (T[mb] > 0).all() and (T[mb] < 6 * 40).all() and T[mb].sum() == 6 * sd.m_below(P)
    n_scans = {Q.n_scan for Q in d.queries}
    assert (max(n_scans) == 129 and {65, 127, 128} <= n_scans) if wide else max(n_scans) == 64
    Ms = [Q.M for Q in d.queries]
    assert len(set(Ms)) == 5 and list(dict.fromkeys(Ms))[4] == sd.m_below(P) == d.queries[mb].M and Ms.count(sd.m_below(P)) == 1
    # ... and that fifth M, the one no cut table is cached for, cuts INSIDE every sub-list of its query: none is empty, each
    # one's last posting has list rank >= M (so the shortcut in front of the binary search does not apply), and both
    # outcomes of the search occur -- sub-lists with some and with no posting of rank < M
    cl, _w = d.emb(mb)
    n_inside = 0
    for r in np.searchsorted(d.cluster_ids, cl):
        ids = d.tweet_ids[d.list_offsets[r]:d.list_offsets[r + 1]]
        part = sd.partitions(lib, ids, P)
        for p in range(P):
            ranks = np.nonzero(part == p)[0]
            assert len(ranks) == 40 and ranks[-1] >= sd.m_below(P), (r, p)
            n_inside += int(ranks[0] < sd.m_below(P))
    assert n_inside >= 6
    lens = np.diff(d.list_offsets)
    assert sd.M_ABOVE > max(lens[np.searchsorted(d.cluster_ids, d.emb(q)[0])].max() for q, Q in enumerate(d.queries) if Q.M == sd.M_ABOVE)
    # ---- sub-list length: no (cluster, partition) sub-list of a unit meant for the fast path exceeds 100 postings
    for q, Q in enumerate(d.queries):
        ids, seq = sd.scanned_postings(d, q)
        if Q.n_scan > sd.NSCAN_MAX or len(ids) == 0:
            continue
        part = sd.partitions(lib, ids, P)
        sub = np.bincount(seq.astype(np.int64) * P + part, minlength=Q.n_scan * P).reshape(Q.n_scan, P)
        assert sub[:, T[q] <= cap].max(initial=0) <= sd.SUBLIST_MAX, (q, Q.role)
    # ---- match list: every nm the duplicate regimes call for is reached, whatever the order of arrival
    assert [Q.nm for Q in d.queries if Q.role == "dup"] == sd.dup_nms(cap)
    for q, Q in enumerate(d.queries):
        if Q.role == "dup":
            nm, clean = sd.match_list(lib, d, q, Q.dup_unit, offline=offline)
            assert clean and nm == Q.nm, (q, nm, Q.nm, clean)
            nm_w, clean_w = sd.match_list(lib, d, q, Q.dup_unit, 12, Q.source)
            assert clean_w and nm_w <= nm
    if offline:
        _offline_checks(lib, oracle, d, T)
        return
    # ---- map size and quota, against the oracle
    kl = sd.quota(sd.K_FAST, P)
    for name in ("k24", "k24_window_source"):
        _cfgs, sources, hours = sd.configuration(d, name, 1)
        live = sd.unit_live(lib, d, hours, sources)
        assert (live <= T).all()
        for alg in ONLINE_ALGS:
            cfgs, _s, _h = sd.configuration(d, name, alg)
            for q in range(d.nq):
                cl, w = d.emb(q)
                o_ids, _o_sc, o_msz = oracle.sann_query(cl, w, sources[q], cfgs[q], sd.NOW_MS, d.cluster_ids, d.list_offsets,
                                                        d.tweet_ids, d.scores)
                assert o_msz == live[q].sum(), (name, alg, q, o_msz, live[q])  # (at P = 1: the unit's own count)
                per_unit = np.bincount(sd.partitions(lib, o_ids, P), minlength=P)
                assert per_unit.max(initial=0) <= kl, (name, alg, q, d.queries[q].role, per_unit, kl)
                if d.queries[q].role == "dup" and name == "k24" and alg in (2, 4):
                    # cosine forms: multi-cluster tweets are among the answers, so the fast path's folding and the sums of its
                    # representatives are what gets compared (the other forms rank by score: no such guarantee)
                    r3, r4 = np.searchsorted(d.cluster_ids, cl[3:5])
                    lists = [d.tweet_ids[d.list_offsets[r]:d.list_offsets[r + 1]] for r in (r3, r4)]
                    shared = np.intersect1d(*lists)
                    assert len(shared) == sd.DUP_HI and np.isin(shared, o_ids).any(), (alg, q, shared, o_ids)


def _offline_checks(lib, oracle, d, T):
    """The offline forms: no window; a tweet of norm 0 is planted and dropped; norms are the full embeddings'."""
    assert (d.norms == 0.0).sum() == 1 and d.tweet_ids[d.norms == 0.0][0] == sd.ZERO_NORM_TWEET
    live = sd.unit_live(lib, d, offline=True)
    assert live.sum() == sd.unit_live(lib, d, 175200).sum() - 1
    uniq, first = np.unique(d.tweet_ids, return_index=True)
    rng = np.random.default_rng(1)
    for t in rng.choice(uniq, 50).tolist():  # the norm column against a plain sum in ascending cluster id
        total = 0.0
        for s in d.scores[d.tweet_ids == t].tolist():
            total = total + s * s
        assert (d.norms[d.tweet_ids == t] == total).all()
    # ---- quota: where the top k of either offline form sit
    kl = sd.quota(sd.K_FAST, d.P)
    for alg in (5, 6):
        for q in range(d.nq):
            per_unit = np.bincount(sd.partitions(lib, sd.offline_top(d, q, alg, sd.K_FAST), d.P), minlength=d.P)
            assert per_unit.max(initial=0) <= kl, (alg, q, d.queries[q].role, per_unit, kl)
    # ---- map size: at P = 1 the model's count of live tweets is the number of rows the SQL has for the user
    if d.P == 1:
        for q, rows in enumerate(sd.sql_rows(oracle, d)):
            assert len(rows) == live[q, 0], (q, len(rows), live[q, 0])
            assert [r[0] for r in rows[:sd.K_FAST]] == sd.offline_top(d, q, 5, sd.K_FAST).tolist()
