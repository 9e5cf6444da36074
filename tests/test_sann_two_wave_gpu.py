"""The two-wave units of the id form, unit_fast_kernel<128, 12>, behind the 8 KB Bloom filter (six bits of one word).

Every case is a host-built index of a few thousand postings at SANN_UNIT_CAP=1536 and a handful of queries, run with
SANN_UNIT_WAVES=2 and with 4; each run is compared with the oracle bit for bit (ids, score bits, counts, map sizes), which
geometry ran is read from sann_debug_unit_waves (QueryBatch.unit_waves), and the units that left the fast path are counted.

1. unit sizes at the slot edges of a 128-thread workgroup (T = 1, 127, 128, 129, 1535, 1536; 1537 overflows), at both
   descriptor strides (n_scan = 1, 50, 64 | 65, 128);
2. duplicates through every settle path: a tweet in 2, 6 and 12 scanned clusters (short lists, settled by each of the two
   waves for itself), 13 and 64 entries (sorted in wave 0), 129 entries (the match list overflows), and a unit made of
   duplicated tweets only; k is above the number of tweets, so every tweet's score is in the answer: a missed pair shows;
3. the data cut with 128 lane maxima: k = 400 at P = 1, 2, 4 makes unit_kl = 128 = WG, so rank kl - 1 is the last rank
   there is; a 12 h window removes half of the best cluster's postings, so the cluster-level cut keeps too few and the
   unit cuts again by its data;
4. what must stay on the four-wave 16-byte form: a batch with a LogCosine config, an index without an id column.
"""
import ctypes as C

import numpy as np
import pytest

import _sann_design as sd

pytestmark = pytest.mark.gpu

CAP = 1536
WG = 128  # threads of a two-wave unit


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


# ---------------------------------------------------------------------------------------------------------------------
# a host-built index: queries with clusters of their own, every (cluster, partition) sub-list of a chosen size
class Builder:
    def __init__(self, lib, P, seed):
        self.lib, self.P = lib, P
        self.rng = np.random.default_rng([20261020, P, seed])
        self.streams = [np.asarray(s) for s in sd.streams(lib, P)]
        self.cur = [0] * P
        self.lists = []  # (cluster id, ids)
        self.emb_o, self.emb_c, self.emb_s = [0], [], []

    def take(self, p, n, keep=None):
        """the next n unused ids of partition p (of those that pass `keep`)"""
        s = self.streams[p]
        out = []
        while len(out) < n:
            t = s[self.cur[p]]
            self.cur[p] += 1
            if keep is None or keep(t):
                out.append(t)
        return np.array(out, np.int64)

    def query(self, counts, weights, plant=None, keep=None):
        """counts[n_scan][P] postings per sub-list; plant(sub) may rewrite partition 0's sub-lists (a list over the clusters);
        keep(c) = predicate on the ids of cluster c.  -> the query's number"""
        q = len(self.emb_o) - 1
        n = len(counts)
        sub = [[self.take(p, int(counts[c][p]), None if keep is None else keep(c)) for p in range(self.P)] for c in range(n)]
        if plant is not None:
            col = [sub[c][0] for c in range(n)]
            plant(col)
            for c in range(n):
                sub[c][0] = col[c]
        for c in range(n):
            ids = np.concatenate(sub[c]) if self.P else np.empty(0, np.int64)
            assert len(np.unique(ids)) == len(ids)
            self.lists.append((1000 * q + 1 + c, ids))
            self.emb_c.append(1000 * q + 1 + c)
            self.emb_s.append(float(weights[c]))
        self.emb_o.append(len(self.emb_c))
        return q

    def finish(self):
        offs = np.zeros(len(self.lists) + 1, np.int64)
        offs[1:] = np.cumsum([len(l[1]) for l in self.lists])
        n = int(offs[-1])
        sc = np.exp(self.rng.normal(-2.0, 1.0, n))
        assert len(np.unique(sc)) == n
        tid = np.empty(n, np.int64)
        for i, (_cid, ids) in enumerate(self.lists):  # lists as the store delivers them: score descending, id ascending
            a, b = int(offs[i]), int(offs[i + 1])
            s = np.sort(sc[a:b])[::-1]
            sc[a:b] = s
            tid[a:b] = ids
        csr = (np.array([l[0] for l in self.lists], np.int32), offs, tid, sc)
        emb = (np.array(self.emb_o, np.int64), np.array(self.emb_c, np.int32), np.array(self.emb_s, np.float64))
        return csr, emb


def split(total, n, rot=0):
    out = np.full(n, total // n, np.int64)
    out[(np.arange(total % n) + rot) % n] += 1
    return out


def counts_for(sizes, n_scan):
    """[n_scan][P]: unit p holds sizes[p] postings, spread over the clusters as evenly as they go"""
    return np.stack([split(int(t), n_scan, p) for p, t in enumerate(sizes)], axis=1)


def _cfg(pkg, c):
    return pkg.SimClustersANNConfig(maxNumResults=c.maxNumResults, minScore=c.minScore, maxTopTweetsPerCluster=c.maxTopTweetsPerCluster,
                                    maxScanClusters=c.maxScanClusters, maxTweetCandidateAgeHours=c.maxTweetCandidateAgeHours,
                                    annAlgorithm=pkg.ScoringAlgorithm(c.annAlgorithm))


def both_geometries(pkg, oracle, monkeypatch, index, csr, emb, cfgs, tag, two_wave=True, id_form=True):
    """The batch with SANN_UNIT_WAVES=2 and =4, each against the oracle.  -> {waves asked for: (unit arrays, stats)}"""
    offs, cids, scs = emb
    nq = len(offs) - 1
    want = [oracle.sann_query(cids[offs[q]:offs[q + 1]], scs[offs[q]:offs[q + 1]], None, cfgs[q], sd.NOW_MS, *csr) for q in range(nq)]
    monkeypatch.setenv("SANN_UNIT_CAP", str(CAP))
    out = {}
    for asked in (2, 4):
        monkeypatch.setenv("SANN_UNIT_WAVES", str(asked))
        qb = pkg.QueryBatch(index, offs, cids, scs, [_cfg(pkg, c) for c in cfgs], now_ms=sd.NOW_MS)
        qb.run()
        units = qb.unit_arrays()
        ran = qb.unit_waves()
        used_ids = qb.id_column()[2]
        qb.finish()
        ids, scores, counts, msz = qb.results()
        st = qb.stats()
        qb.close()
        assert ran == (2 if asked == 2 and two_wave else 4, CAP), (tag, asked, ran)
        assert used_ids == id_form, (tag, asked)
        for q, (o_ids, o_sc, o_msz) in enumerate(want):
            assert counts[q] == len(o_ids), (tag, asked, q, counts[q], len(o_ids))
            assert msz[q] == o_msz, (tag, asked, q, msz[q], o_msz)
            assert np.array_equal(ids[q, :counts[q]], o_ids), (tag, asked, q, "id order differs")
            assert np.array_equal(scores[q, :counts[q]].view(np.int64), np.asarray(o_sc).view(np.int64)), (tag, asked, q, "scores differ")
        out[asked] = (units, st)
    monkeypatch.delenv("SANN_UNIT_WAVES")
    return out


def overflowed(units):
    return (units[3] & sd.UNIT_OVERFLOW) != 0


# ---------------------------------------------------------------------------------------------------------------------
# 1. slot edges
SMALL, LARGE = (1, 127, 128, 129), (1535, 1536, 1537, 64)


@pytest.mark.parametrize("n_scan", [1, 50, 64, 65, 128])
def test_unit_sizes_at_the_slot_edges(pkg, oracle, lib, monkeypatch, n_scan):
    P = 4
    b = Builder(lib, P, n_scan)
    n_large = max(n_scan, 50)  # (one cluster of 1536 postings would be ONE key: a tie group no survivor list holds)
    b.query(counts_for(SMALL, n_scan), np.exp(b.rng.normal(0.0, 0.5, n_scan)))
    b.query(counts_for(LARGE, n_large), np.exp(b.rng.normal(0.0, 0.5, n_large)))
    csr, emb = b.finish()
    index = pkg.ClusterTweetIndex(*csr, n_partitions=P)
    for alg in (2, 4):
        cfgs = [sd.Cfg(40, 20000, 24, alg)] * 2
        runs = both_geometries(pkg, oracle, monkeypatch, index, csr, emb, cfgs, (n_scan, alg))
        for asked, (units, st) in runs.items():
            assert np.array_equal(units[0], np.array([SMALL, LARGE])), (asked, units[0])
            over = overflowed(units)
            assert over.sum() == 1 and over[1, 2], (asked, np.argwhere(over).tolist())  # T = 1537 alone
            assert st.n_fallback_units == 1 and st.n_requeried == 0, (asked, st.n_fallback_units, st.n_requeried)
            assert np.array_equal(units[1][~over], units[0][~over])  # (no duplicate: every posting a live tweet)
    index.close()


def test_two_waves_are_the_default(pkg, lib, monkeypatch):
    b = Builder(lib, 4, 0)
    b.query(counts_for((100, 200, 300, 400), 20), np.linspace(1.0, 0.5, 20))
    csr, emb = b.finish()
    index = pkg.ClusterTweetIndex(*csr, n_partitions=4)
    monkeypatch.delenv("SANN_UNIT_WAVES", raising=False)
    cfg = _cfg(pkg, sd.Cfg(40, 20000, 24, 2))
    for cap, want in ((CAP, 2), (1024, 4), (3072, 4), (512, 2), (256, 1)):
        monkeypatch.setenv("SANN_UNIT_CAP", str(cap))
        qb = pkg.QueryBatch(index, *emb, cfg, now_ms=sd.NOW_MS)
        assert qb.unit_waves()[0] == 0  # (nothing ran yet)
        qb.run()
        qb.finish()
        assert qb.unit_waves() == (want, cap)
        qb.close()
    index.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. duplicates
def planter(b, mults):
    """mults = in how many clusters each planted tweet sits; clusters are taken round robin, a cluster's slots from its front"""
    def plant(col):
        n = len(col)
        used = [0] * n
        c = 0
        for m in mults:
            assert m <= n
            t = b.take(0, 1)[0]
            for i in range(m):
                cl = (c + i) % n
                assert used[cl] < len(col[cl])
                col[cl][used[cl]] = t
                used[cl] += 1
            c = (c + m) % n
    return plant


DUPS = [("one tweet in 2 clusters", [2]), ("one tweet in 6", [6]), ("one tweet in 12", [12]), ("13 entries", [2, 2, 2, 2, 2, 3]),
        ("64 entries", [2] * 32), ("129 entries", [3] * 43)]


@pytest.mark.parametrize("wide", [False, True], ids=["ns64", "ns128"])
def test_duplicates_through_every_settle_path(pkg, oracle, lib, monkeypatch, wide):
    P, n, L = 4, 16, 9  # 144 postings per unit: under keep_all = 160, so a unit offers every tweet it holds
    b = Builder(lib, P, 100 + int(wide))
    for _name, mults in DUPS:
        b.query(np.full((n, P), L), np.exp(b.rng.normal(0.0, 0.5, n)), plant=planter(b, mults))
    q_all = b.query(np.full((4, P), 30), np.exp(b.rng.normal(0.0, 0.5, 4)), plant=planter(b, [2] * 60))  # unit 0: pairs only
    if wide:
        b.query(counts_for((65, 66, 67, 68), 65), np.exp(b.rng.normal(0.0, 0.5, 65)))
    csr, emb = b.finish()
    nq = len(emb[0]) - 1
    index = pkg.ClusterTweetIndex(*csr, n_partitions=P)
    for alg in (2, 4):
        cfgs = [sd.Cfg(1000, 20000, 24, alg)] * nq
        runs = both_geometries(pkg, oracle, monkeypatch, index, csr, emb, cfgs, ("dups", wide, alg))
        for asked, (units, st) in runs.items():
            T, uniq, cnt, _flags = units
            over = overflowed(units)
            assert over.sum() == 1 and over[5, 0], (asked, np.argwhere(over).tolist())  # the 129-entry match list alone
            assert st.n_fallback_units == 1 and st.n_requeried == 0, (asked, st.n_fallback_units, st.n_requeried)
            for q, (_name, mults) in enumerate(DUPS[:5]):
                assert T[q, 0] == n * L and uniq[q, 0] == n * L - sum(mults) + len(mults), (asked, q, uniq[q, 0])
                assert cnt[q, 0] == uniq[q, 0], (asked, q, "a unit under keep_all offers every tweet")
            assert T[q_all, 0] == 120 and uniq[q_all, 0] == 60 and cnt[q_all, 0] == 60, (asked, uniq[q_all, 0], cnt[q_all, 0])
    index.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the data cut with as many lane maxima as unit_kl
@pytest.mark.parametrize("P", [1, 2, 4])
def test_data_cut_with_128_lane_maxima(pkg, oracle, lib, monkeypatch, P):
    """25 clusters of 16 postings per unit, weights falling with the cluster: the cluster-level cut covers kl = 128 postings
    with the eight best clusters, the window then removes 8 of the best cluster's 16, and 120 < kl survive: the unit cuts by
    its data.  Its 128 lane maxima: a thread whose first posting fell to the window has its best in cluster 8 (posting
    t + 128), so the 128th largest maximum is cluster 8's key and clusters 0 ... 8 survive: 8 + 8 * 16 = 136 candidates."""
    k, n, L = 400, 25, 16
    assert sd.unit_kl(k, P) == WG
    lo12, _hi = sd.window(12)
    b = Builder(lib, P, 200 + P)
    half = [0]

    def keep(c):
        if c != 0:
            return lambda t: t >= lo12
        def alternate(t):  # cluster 0: old and young ids in turns
            ok = (t < lo12) == (half[0] % 2 == 0)
            half[0] += int(ok)
            return ok
        return alternate

    b.query(np.full((n, P), L), 1.0 - 0.02 * np.arange(n), keep=keep)
    csr, emb = b.finish()
    old = csr[2] < lo12
    assert old.sum() == 8 * P and old[:16 * P].sum() == 8 * P
    index = pkg.ClusterTweetIndex(*csr, n_partitions=P)
    for alg in (2, 4):
        runs = both_geometries(pkg, oracle, monkeypatch, index, csr, emb, [sd.Cfg(k, 20000, 12, alg)], ("data cut", P, alg))
        for asked, (units, st) in runs.items():
            T, uniq, cnt, _flags = units
            assert not overflowed(units).any(), asked
            assert (T == n * L).all() and (uniq == n * L - 8).all(), (asked, T, uniq)
            assert (cnt == 136).all(), (asked, cnt)
            # P units of at most 160 candidates cannot prove 400 answers at P = 1, 2: the query is answered by the general
            # path; at P = 4 the 400th answer lies in cluster 6, above every unit's cut
            assert (st.n_requeried, st.n_fallback_units) == ((0, 0) if P == 4 else (1, P)), (asked, st.n_requeried, st.n_fallback_units)
    index.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. batches that have no two-wave form
def _plain(lib, P, seed):
    b = Builder(lib, P, seed)
    for i in range(3):
        b.query(counts_for((1500, 1400, 1300, 129), 50), np.exp(b.rng.normal(0.0, 0.5, 50)), plant=planter(b, [2, 2, 3]))
    return b.finish()


def test_mixed_batch_keeps_the_four_wave_16_byte_form(pkg, oracle, lib, monkeypatch):
    csr, emb = _plain(lib, 4, 300)
    index = pkg.ClusterTweetIndex(*csr, n_partitions=4)
    cfgs = [sd.Cfg(40, 20000, 24, 2), sd.Cfg(40, 20000, 24, 3), sd.Cfg(40, 20000, 24, 4)]  # LogCosine among the cosine forms
    runs = both_geometries(pkg, oracle, monkeypatch, index, csr, emb, cfgs, "mixed", two_wave=False, id_form=False)
    for asked, (units, st) in runs.items():
        # (no unit left the fast path on its own; a query the merge could not prove is answered again, all its units with it)
        assert not overflowed(units).any() and st.n_fallback_units == 4 * st.n_requeried, (asked, st.n_fallback_units, st.n_requeried)
    # cosine alone: the same index takes the two-wave form
    runs = both_geometries(pkg, oracle, monkeypatch, index, csr, emb, [cfgs[0]] * 3, "cosine alone")
    for asked, (units, st) in runs.items():
        # (no unit left the fast path on its own; a query the merge could not prove is answered again, all its units with it)
        assert not overflowed(units).any() and st.n_fallback_units == 4 * st.n_requeried, (asked, st.n_fallback_units, st.n_requeried)
    index.close()


def test_index_without_id_column_keeps_the_four_wave_form(pkg, oracle, lib, monkeypatch):
    sa = pkg.simclusters_ann
    csr, emb = _plain(lib, 4, 301)
    cl, lo, tid, sc = csr
    post = np.zeros(len(tid), np.dtype([("id", np.int64), ("score", np.float64)]))
    post["id"], post["score"] = tid, sc
    d_post = C.c_void_p()
    assert lib.sann_device_alloc(0, max(post.nbytes, 16), C.byref(d_post)) == 0, lib.sann_last_error()
    assert lib.sann_device_copy(0, d_post, post.ctypes.data_as(C.c_void_p), post.nbytes) == 0, lib.sann_last_error()
    opts = sa.sann_index_options_t(0, 4, 0, 1)
    h = C.c_void_p()
    cl, lo = np.ascontiguousarray(cl, np.int32), np.ascontiguousarray(lo, np.int64)
    rc = lib.sann_index_build_from_device_postings(C.byref(opts), len(cl), cl.ctypes.data_as(C.c_void_p), lo.ctypes.data_as(C.c_void_p), d_post, C.byref(h))
    assert rc == 0, lib.sann_last_error()
    index = sa.ClusterTweetIndex.__new__(sa.ClusterTweetIndex)
    index._h, index.device, index.cluster_ids, index.list_offsets = h, 0, cl, lo
    runs = both_geometries(pkg, oracle, monkeypatch, index, csr, emb, [sd.Cfg(40, 20000, 24, 2)] * 3, "no column", two_wave=False, id_form=False)
    for asked, (units, st) in runs.items():
        # (no unit left the fast path on its own; a query the merge could not prove is answered again, all its units with it)
        assert not overflowed(units).any() and st.n_fallback_units == 4 * st.n_requeried, (asked, st.n_fallback_units, st.n_requeried)
    index.close()
    assert lib.sann_device_free(0, d_post) == 0
