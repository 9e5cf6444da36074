"""The two-wave id-form units find a posting's cluster by a bit count: one end bit per non-empty cluster's stretch in a
1536-bit map, the cluster's RANK among the unit's non-empty clusters from the bits below the posting, the unit's tables
(offsets, weights, keys) indexed by rank, and the cluster itself named only where a survivor leaves the unit.

Every case is a host-built index of a few thousand postings at SANN_UNIT_CAP=1536, P = 4, algorithms 2 and 4, run with the
default (32-bit) offsets and with SANN_UNIT_OFFSETS=64; each run is compared with the oracle bit for bit (ids, score bits,
counts, map sizes) and must have run as two-wave units of 1536.  Cluster weights are pairwise distinct, so a posting given
a neighbour's weight changes score bits; where duplicates are planted k is above the number of tweets, so a missed or
doubled tweet shows.  Sub-list sizes are explicit counts[n_scan][P], zeros included.

1. stretches that end at flat indices 0, 62, 63, 64, 65, 127, 128, 1534 and 1535, a cluster that spans three words, one-posting
   clusters on either side of a word boundary, 64 clusters of 24 and (128-cluster stride) 128 clusters of 12;
2. empty sub-lists, so that rank != cluster: the first, the last, a run of five, every second cluster empty; a unit whose
   only non-empty cluster is the last; a unit with T = 0 beside non-empty ones; n_scan = 1, 50, 64 | 65, 128;
3. duplicates across empty clusters: one tweet in clusters 0, 5 and 9 with the clusters between them empty, as 1, 4, 13, 21
   and 36 groups (3 and 12 entries: every wave settles for itself; 39 and 63: sorted in wave 0; 108: the pairwise pass), in
   units under keep_all, so unit_unique is exact;
4. a survivor of the cluster-level cut from a cluster whose rank differs from its number;
5. T = 1537 goes to the general path, the query's other units do not;
6. a query whose sub-lists are the index's last postings, units ending inside a slot: the spare table entry.
"""
import numpy as np
import pytest

import _sann_design as sd
from test_sann_two_wave_gpu import Builder, _cfg, counts_for, overflowed, planter

pytestmark = pytest.mark.gpu

CAP = 1536
P = 4


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def both_offsets(pkg, oracle, monkeypatch, index, csr, emb, cfgs, tag):
    """The batch with the default offsets and with SANN_UNIT_OFFSETS=64, each against the oracle.
    -> {bits: (unit arrays, stats)}"""
    offs, cids, scs = emb
    nq = len(offs) - 1
    want = [oracle.sann_query(cids[offs[q]:offs[q + 1]], scs[offs[q]:offs[q + 1]], None, cfgs[q], sd.NOW_MS, *csr) for q in range(nq)]
    monkeypatch.setenv("SANN_UNIT_CAP", str(CAP))
    monkeypatch.delenv("SANN_UNIT_WAVES", raising=False)
    out = {}
    for bits in (32, 64):
        if bits == 64:
            monkeypatch.setenv("SANN_UNIT_OFFSETS", "64")
        else:
            monkeypatch.delenv("SANN_UNIT_OFFSETS", raising=False)
        qb = pkg.QueryBatch(index, offs, cids, scs, [_cfg(pkg, c) for c in cfgs], now_ms=sd.NOW_MS)
        qb.run()
        units = qb.unit_arrays()
        ran = (qb.unit_waves(), qb.unit_offsets(), qb.id_column()[2])
        qb.finish()
        ids, scores, counts, msz = qb.results()
        st = qb.stats()
        qb.close()
        assert ran == ((2, CAP), bits, True), (tag, bits, ran)
        for q, (o_ids, o_sc, o_msz) in enumerate(want):
            assert counts[q] == len(o_ids), (tag, bits, q, counts[q], len(o_ids))
            assert msz[q] == o_msz, (tag, bits, q, msz[q], o_msz)
            assert np.array_equal(ids[q, :counts[q]], o_ids), (tag, bits, q, "id order differs")
            assert np.array_equal(scores[q, :counts[q]].view(np.int64), np.asarray(o_sc).view(np.int64)), (tag, bits, q, "scores differ")
        out[bits] = (units, st)
    monkeypatch.delenv("SANN_UNIT_OFFSETS", raising=False)
    return out


def distinct_weights(b, n, lowest=()):
    """n pairwise distinct weights in random order; the clusters of `lowest` get the smallest of them"""
    w = np.exp(b.rng.normal(0.0, 0.5, n))
    assert len(np.unique(w)) == n
    order = np.argsort(w)
    for i, c in enumerate(lowest):
        j = int(order[i])
        w[[c, j]] = w[[j, c]]
        order = np.argsort(w)
    return w


def with_empty_rows(counts, rows):
    """counts[n][P] with all-zero rows inserted so that they end up at the indices `rows`"""
    counts = np.asarray(counts)
    n = len(counts) + len(rows)
    out = np.zeros((n, counts.shape[1]), np.int64)
    out[[c for c in range(n) if c not in set(rows)]] = counts
    return out


def run_and_check_sizes(pkg, oracle, monkeypatch, b, queries, k, tag, fallback=None):
    """queries = [counts[n][P] per query, in the order they were added].  Both offsets, both algorithms; every unit's T is the
    planted size; no unit leaves the fast path on its own unless `fallback` = (query, partition) names the one that must."""
    csr, emb = b.finish()
    nq = len(emb[0]) - 1
    assert nq == len(queries)
    planted = np.array([np.asarray(c).sum(axis=0) for c in queries])
    index = pkg.ClusterTweetIndex(*csr, n_partitions=P)
    runs_by_alg = {}
    for alg in (2, 4):
        runs = both_offsets(pkg, oracle, monkeypatch, index, csr, emb, [sd.Cfg(k, 20000, 24, alg)] * nq, (tag, alg))
        for bits, (units, st) in runs.items():
            assert np.array_equal(units[0], planted), (tag, alg, bits, units[0], planted)
            over = overflowed(units)
            if fallback is None:
                assert not over.any(), (tag, alg, bits, np.argwhere(over).tolist())
                assert st.n_fallback_units == P * st.n_requeried, (tag, alg, bits, st.n_fallback_units, st.n_requeried)
            else:
                assert over.sum() == 1 and over[fallback], (tag, alg, bits, np.argwhere(over).tolist())
                assert st.n_fallback_units == 1 and st.n_requeried == 0, (tag, alg, bits, st.n_fallback_units, st.n_requeried)
        runs_by_alg[alg] = runs
    index.close()
    return runs_by_alg


# ---------------------------------------------------------------------------------------------------------------------
# 1. stretch ends at word edges
# sub-list lengths of one unit: stretches end at 0, 62, 63, 64, 65, 127, 128, then a cluster of 200 (three words and more),
# then 62s up to 1534 and a last cluster of one posting at 1535
EDGE_LENGTHS = [1, 62, 1, 1, 1, 62, 1, 200] + [62] * 19 + [28, 1]
LONG = 7  # (the long cluster is ONE key: it gets the lowest weight, so that no cut falls into a tie group of 200)


def test_edge_lengths_are_what_they_claim():
    ends = np.cumsum(EDGE_LENGTHS) - 1
    assert set((0, 62, 63, 64, 65, 127, 128, 1534, 1535)) <= set(ends.tolist()) and ends[-1] == CAP - 1
    assert EDGE_LENGTHS[LONG] >= 130 and ends[LONG] // 64 - (ends[LONG - 1] + 1) // 64 >= 2 and max(EDGE_LENGTHS[:LONG] + EDGE_LENGTHS[LONG + 1:]) <= 62


@pytest.mark.parametrize("wide", [False, True], ids=["ns64", "ns128"])
def test_stretch_ends_at_word_edges(pkg, oracle, lib, monkeypatch, wide):
    n = len(EDGE_LENGTHS)
    b = Builder(lib, P, 800 + int(wide))
    # partition 0: the lengths; 1: the same backwards; 2: one posting per cluster (a boundary between any two); 3: two
    edge = np.stack([EDGE_LENGTHS, EDGE_LENGTHS[::-1], [1] * n, [2] * n], axis=1)
    queries = []
    for _variant in range(3):  # three weight orders: which clusters the cut keeps differs
        b.query(edge, distinct_weights(b, n, lowest=(LONG, n - 1 - LONG)))
        queries.append(edge)
    if wide:
        c = with_empty_rows(edge, list(range(n, n + 40)))  # the same units at the 128-cluster stride
        b.query(c, distinct_weights(b, len(c), lowest=(LONG, n - 1 - LONG)))
        queries.append(c)
        c = np.full((128, P), 12)  # T = 1536 made of 128 clusters of 12
    else:
        c = np.full((64, P), 24)  # T = 1536 made of 64 clusters of 24
    b.query(c, distinct_weights(b, len(c)))
    queries.append(c)
    run_and_check_sizes(pkg, oracle, monkeypatch, b, queries, 40, ("edges", wide))


# ---------------------------------------------------------------------------------------------------------------------
# 2. empty sub-lists
@pytest.mark.parametrize("n_scan", [1, 50, 64, 65, 128])
def test_empty_sub_lists(pkg, oracle, lib, monkeypatch, n_scan):
    n = n_scan
    L = 20 if n <= 64 else 9
    b = Builder(lib, P, 900 + n_scan)
    queries = []
    if n == 1:
        queries.append(np.array([[0, 7, 0, 30]]))  # units with T = 0 beside non-empty ones
        queries.append(np.array([[129, 0, 1, 0]]))
    else:
        c = np.full((n, P), L)
        c[0, 0] = 0                      # partition 0: the first cluster empty
        c[n - 1, 1] = 0                  # 1: the last
        c[n // 2:n // 2 + 5, 2] = 0      # 2: a run of five in the middle
        c[1::2, 3] = 0                   # 3: every second
        queries.append(c)
        c = np.full((n, P), L)
        c[:, 0] = 0
        c[n - 1, 0] = 30                 # partition 0: a single non-empty cluster, the last one
        c[:, 1] = 0                      # 1: T = 0
        c[::2, 2] = 0                    # 2: every second, the other parity
        c[:n - 3, 3] = [(i * 7) % 23 for i in range(n - 3)]  # 3: sizes 0 ... 22 in no order
        queries.append(c)
    for c in queries:
        b.query(c, distinct_weights(b, n))
    run_and_check_sizes(pkg, oracle, monkeypatch, b, queries, 40, ("empty", n_scan))


# ---------------------------------------------------------------------------------------------------------------------
# 3. duplicates across empty clusters
SPREAD = (0, 5, 9)  # the clusters a planted tweet sits in; 1-4 and 6-8 are empty in its partition
GROUPS = (1, 4, 13, 21, 36)  # (36: 108 entries of the match list's 128, room for a false flag or two)


def plant_spread(b, groups):
    def plant(col):
        for g in range(groups):
            t = b.take(0, 1)[0]
            for c in SPREAD:
                col[c][g] = t
    return plant


@pytest.mark.parametrize("wide", [False, True], ids=["ns64", "ns128"])
def test_duplicates_across_empty_clusters(pkg, oracle, lib, monkeypatch, wide):
    n = 16
    b = Builder(lib, P, 1000 + int(wide))
    queries = []
    for g in GROUPS:
        c = np.full((n, P), 9)
        c[:, 0] = 5
        c[1:9, 0] = 0
        c[list(SPREAD), 0] = g + 2
        b.query(c, distinct_weights(b, n), plant=plant_spread(b, g))
        queries.append(c)
    if wide:
        c = counts_for((65, 66, 67, 68), 65)
        b.query(c, distinct_weights(b, 65))
        queries.append(c)
    runs_by_alg = run_and_check_sizes(pkg, oracle, monkeypatch, b, queries, 1000, ("spread", wide))
    for alg, runs in runs_by_alg.items():
        for bits, (units, _st) in runs.items():
            T, uniq, cnt, _flags = units
            for q, g in enumerate(GROUPS):
                assert T[q, 0] == 3 * (g + 2) + 30 and uniq[q, 0] == T[q, 0] - 2 * g, (alg, bits, q, T[q, 0], uniq[q, 0])
                assert (uniq[q, 1:] == T[q, 1:]).all(), (alg, bits, q, uniq[q])
                assert (cnt[q] == uniq[q]).all(), (alg, bits, q, "a unit under keep_all offers every tweet", cnt[q], uniq[q])


# ---------------------------------------------------------------------------------------------------------------------
# 4. the hand-over names the cluster, not the rank
def test_survivor_from_a_cluster_whose_rank_is_not_its_number(pkg, oracle, lib, monkeypatch):
    n = 20
    b = Builder(lib, P, 1100)
    c = np.full((n, P), 20)
    c[:5, 0] = 0        # partition 0: rank = cluster - 5
    c[::2, 1] = 0       # 1: rank = cluster / 2
    c[3, 2] = 0         # 2: rank = cluster - 1 from cluster 4 on
    queries = [c, c]
    b.query(c, distinct_weights(b, n))
    b.query(c, np.linspace(0.5, 1.5, n))  # the best clusters are the last: the largest gap between rank and cluster
    runs_by_alg = run_and_check_sizes(pkg, oracle, monkeypatch, b, queries, 40, "hand-over")
    keep_all = sd.unit_kl(40, P) + sd.unit_kl(40, P) // 2 + 16
    for alg, runs in runs_by_alg.items():
        for bits, (units, _st) in runs.items():
            T, uniq, cnt, _flags = units
            assert (uniq == T).all() and (T > keep_all).all(), (alg, bits, T)
            assert (cnt < uniq).all(), (alg, bits, "the cluster-level cut is in force", cnt, uniq)


# ---------------------------------------------------------------------------------------------------------------------
# 5. overflow
def test_oversized_unit_beside_full_ones(pkg, oracle, lib, monkeypatch):
    b = Builder(lib, P, 1200)
    sizes = (1535, 1536, 1537, 64)
    c = with_empty_rows(counts_for(sizes, 45), [0, 10, 11, 12, 49])
    b.query(c, distinct_weights(b, len(c)))
    small = counts_for((300, 300, 300, 300), 20)
    b.query(small, distinct_weights(b, 20))
    run_and_check_sizes(pkg, oracle, monkeypatch, b, [c, small], 40, "overflow", fallback=(0, 2))


# ---------------------------------------------------------------------------------------------------------------------
# 6. the index's last postings
def test_query_at_the_end_of_the_index(pkg, oracle, lib, monkeypatch):
    b = Builder(lib, P, 1300)
    first = counts_for((300, 300, 300, 300), 20)
    b.query(first, distinct_weights(b, 20))
    sizes = (5, 130, 700, 1300)  # none a multiple of 64: every unit ends inside a slot, and inside a word
    c = with_empty_rows(counts_for(sizes, 45), [0, 20, 21, 22, 23])
    c[-1, 3] += c[-2, 3]  # partition 3 (the index's very last postings): the last but one cluster empty as well
    c[-2, 3] = 0
    for p in range(P):  # every unit's last posting lies in the index's last list
        if c[-1, p] == 0:
            c[np.flatnonzero(c[:, p])[0], p] -= 1
            c[-1, p] += 1
    q = b.query(c, distinct_weights(b, len(c)))
    assert c[-1].min() > 0 and tuple(c.sum(axis=0)) == sizes
    lists = b.lists
    assert lists[-1][0] == 1000 * q + len(c)  # the query's last cluster is the index's last list
    run_and_check_sizes(pkg, oracle, monkeypatch, b, [first, c], 40, "last row")
