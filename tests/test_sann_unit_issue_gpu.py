"""The two-wave id-form units after round 12's cuts of issue slots per posting slot: 32-bit gather offsets from the id
column's base, word and bits of the 8 KB filter from one product, zero-mask atomics in dead slots.

Every case is a host-built index of a few thousand postings at SANN_UNIT_CAP=1536 and a handful of queries, run with the
default (32-bit offsets) and with SANN_UNIT_OFFSETS=64; each run is compared with the oracle bit for bit (ids, score bits,
counts, map sizes), and which form ran is read from sann_debug_unit_waves / sann_debug_unit_offsets.

1. unit sizes at the slot edges of a 128-thread workgroup (T = 1, 127, 128, 129, 1280, 1281, 1535, 1536; 1537 overflows to the
   general path), at both descriptor strides (n_scan = 1, 50, 64 | 65, 128);
2. a query whose sub-lists are the index's last postings and whose units all end inside a slot: the clamped slots re-read
   the index's last row;
3. duplicates through the changed mask code: a tweet in 2, 6, 12, 13 and 64 scanned clusters, two postings of one tweet in
   one thread's slots and in different waves, a unit of duplicated tweets only, and ids chosen to share a filter word and
   to cover each other's bits (false flags); k is above the number of tweets, so a missed pair shows;
4. a 12 h window that removes half of every unit's slots (dead slots take the zero-mask atomic) and a source-tweet hit.
"""
import numpy as np
import pytest

import _sann_design as sd
from test_sann_two_wave_gpu import Builder, _cfg, counts_for, overflowed, planter

pytestmark = pytest.mark.gpu

CAP = 1536
M32 = np.uint64(0xFFFFFFFF)


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def both_offsets(pkg, oracle, monkeypatch, index, csr, emb, cfgs, tag, sources=None):
    """The batch with the default offsets and with SANN_UNIT_OFFSETS=64, each against the oracle.
    -> {bits: (unit arrays, stats)}"""
    offs, cids, scs = emb
    nq = len(offs) - 1
    sources = sources or [None] * nq
    want = [oracle.sann_query(cids[offs[q]:offs[q + 1]], scs[offs[q]:offs[q + 1]], sources[q], cfgs[q], sd.NOW_MS, *csr) for q in range(nq)]
    monkeypatch.setenv("SANN_UNIT_CAP", str(CAP))
    monkeypatch.delenv("SANN_UNIT_WAVES", raising=False)
    src = np.array([0 if s is None else s for s in sources], np.int64)
    has = np.array([0 if s is None else 1 for s in sources], np.uint8)
    out = {}
    for bits in (32, 64):
        if bits == 64:
            monkeypatch.setenv("SANN_UNIT_OFFSETS", "64")
        else:
            monkeypatch.delenv("SANN_UNIT_OFFSETS", raising=False)
        qb = pkg.QueryBatch(index, offs, cids, scs, [_cfg(pkg, c) for c in cfgs], now_ms=sd.NOW_MS, source_tweet_ids=src, has_source_tweet=has)
        assert qb.unit_offsets() == 0  # (nothing ran yet)
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


# ---------------------------------------------------------------------------------------------------------------------
# 1. slot edges
SMALL, LARGE, OVER = (1, 127, 128, 129), (1280, 1281, 1535, 1536), (1535, 1536, 1537, 64)


@pytest.mark.parametrize("n_scan", [1, 50, 64, 65, 128])
def test_unit_sizes_at_the_slot_edges(pkg, oracle, lib, monkeypatch, n_scan):
    P = 4
    b = Builder(lib, P, 400 + n_scan)
    n_large = max(n_scan, 50)  # (one cluster of 1536 postings would be ONE key: a tie group no survivor list holds)
    b.query(counts_for(SMALL, n_scan), np.exp(b.rng.normal(0.0, 0.5, n_scan)))
    b.query(counts_for(LARGE, n_large), np.exp(b.rng.normal(0.0, 0.5, n_large)))
    # (the oversized unit among large ones: the rest of its query still offers enough to prove the answer without it)
    b.query(counts_for(OVER, n_large), np.exp(b.rng.normal(0.0, 0.5, n_large)))
    csr, emb = b.finish()
    index = pkg.ClusterTweetIndex(*csr, n_partitions=P)
    for alg in (2, 4):
        runs = both_offsets(pkg, oracle, monkeypatch, index, csr, emb, [sd.Cfg(40, 20000, 24, alg)] * 3, (n_scan, alg))
        for bits, (units, st) in runs.items():
            assert np.array_equal(units[0], np.array([SMALL, LARGE, OVER])), (bits, units[0])
            over = overflowed(units)
            assert over.sum() == 1 and over[2, 2], (bits, np.argwhere(over).tolist())  # T = 1537 alone
            assert st.n_fallback_units == 1 and st.n_requeried == 0, (bits, st.n_fallback_units, st.n_requeried)
            assert np.array_equal(units[1][~over], units[0][~over])  # (no duplicate: every posting a live tweet)
    index.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the index's last row
def test_query_at_the_end_of_the_index(pkg, oracle, lib, monkeypatch):
    P = 4
    b = Builder(lib, P, 500)
    b.query(counts_for((300, 300, 300, 300), 20), np.exp(b.rng.normal(0.0, 0.5, 20)))
    sizes = (5, 130, 700, 1300)  # none a multiple of 128: every unit's last slot is clamped to its last posting
    q = b.query(counts_for(sizes, 50), np.exp(b.rng.normal(0.0, 0.5, 50)))
    csr, emb = b.finish()
    assert emb[1][emb[0][q]:emb[0][q + 1]].max() == csr[0][-1]  # the query's last cluster is the index's last list
    index = pkg.ClusterTweetIndex(*csr, n_partitions=P)
    for alg in (2, 4):
        runs = both_offsets(pkg, oracle, monkeypatch, index, csr, emb, [sd.Cfg(40, 20000, 24, alg)] * 2, ("last row", alg))
        for bits, (units, st) in runs.items():
            assert np.array_equal(units[0][q], np.array(sizes)), (bits, units[0])
            assert not overflowed(units).any() and st.n_fallback_units == 4 * st.n_requeried, (bits, st.n_fallback_units, st.n_requeried)
    index.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. duplicates
def bloom_product(ids):
    """csrc/sann_unit.h bloom_fold / bloom_product / bloom_product_bits -> (filter word, 64-bit mask)"""
    u = np.asarray(ids, np.int64).view(np.uint64)
    x = (u ^ (u >> np.uint64(32))) & M32
    x ^= x >> np.uint64(15)
    p = x * np.uint64(0x9E3779B1)
    lo, hi = p & M32, p >> np.uint64(32)
    one = np.uint64(1)
    f = lambda s: one << ((hi >> np.uint64(s)) & np.uint64(31))
    return (lo >> np.uint64(22)).astype(np.int64), ((f(15) | f(20) | f(25)) << np.uint64(32)) | f(0) | f(5) | f(10)


def covered_core(ids):
    """the largest subset of ids (of one filter word) in which every id's mask is covered by the others' masks"""
    ids = np.asarray(ids, np.int64)
    while len(ids):
        mask = bloom_product(ids)[1]
        ok = np.array([mask[j] & ~np.bitwise_or.reduce(np.delete(mask, j)) == 0 for j in range(len(ids))])
        if ok.all():
            break
        ids = ids[ok]
    return ids


def plant_pairs(b, pairs):
    """pairs = ((cluster, cluster, slot), ...): one new tweet at the same slot of both clusters' partition-0 sub-lists"""
    def plant(col):
        for c1, c2, i in pairs:
            col[c1][i] = col[c2][i] = b.take(0, 1)[0]
    return plant


DUPS = [("one tweet in 2 clusters", [2]), ("one tweet in 6", [6]), ("one tweet in 12", [12]), ("13 entries", [2, 2, 2, 2, 2, 3]),
        ("64 entries", [2] * 32)]


def test_duplicates_through_the_mask_code(pkg, oracle, lib, monkeypatch):
    P, n, L = 4, 18, 8  # 144 postings per unit: under keep_all = 160, so a unit offers every tweet it holds
    b = Builder(lib, P, 600)
    w = lambda k: np.exp(b.rng.normal(0.0, 0.5, k))
    for _name, mults in DUPS:
        b.query(np.full((n, P), L), w(n), plant=planter(b, mults))
    # flat posting j of a unit sits in slot j / 128 of thread j % 128: clusters 16 apart share a thread, 8 apart do not share a wave
    q_thread = b.query(np.full((n, P), L), w(n), plant=plant_pairs(b, ((0, 16, 3), (1, 17, 5))))
    q_waves = b.query(np.full((n, P), L), w(n), plant=plant_pairs(b, ((0, 8, 3), (2, 10, 7))))
    q_all = b.query(np.full((4, P), 30), w(4), plant=planter(b, [2] * 60))  # unit 0: pairs only
    q_64 = b.query(np.full((64, P), 2), w(64), plant=planter(b, [64]))    # one tweet in 64 scanned clusters
    # false flags: per unit, distinct ids that share ONE filter word and each of whose masks the others' masks cover --
    # whichever of them arrives last finds its six bits set
    rest = [s[b.cur[p]:] for p, s in enumerate(b.streams)]
    words = [bloom_product(r)[0] for r in rest]
    word = int(np.argmax(np.min([np.bincount(x, minlength=1024) for x in words], axis=0)))
    cores = [covered_core(r[x == word]) for r, x in zip(rest, words)]
    assert min(len(c) for c in cores) >= 16, [len(c) for c in cores]
    good = set(np.concatenate(cores).tolist())
    q_false = b.query(counts_for([len(c) for c in cores], 4), w(4), keep=lambda c: good.__contains__)
    csr, emb = b.finish()
    offs = emb[0]
    nq = len(offs) - 1
    lists = {cid: ids for cid, ids in b.lists}
    mine = np.concatenate([lists[c] for c in emb[1][offs[q_false]:offs[q_false + 1]]])
    part = sd.partitions(lib, mine, P)
    for p in range(P):
        wd, mask = bloom_product(mine[part == p])
        assert len(mask) == len(cores[p]) and (wd == word).all()
        for j in range(len(mask)):
            assert mask[j] & ~np.bitwise_or.reduce(np.delete(mask, j)) == 0, "the unit's last arrival must find all its bits set"
    index = pkg.ClusterTweetIndex(*csr, n_partitions=P)
    for alg in (2, 4):
        cfgs = [sd.Cfg(1000, 20000, 24, alg)] * nq
        runs = both_offsets(pkg, oracle, monkeypatch, index, csr, emb, cfgs, ("dups", alg))
        for bits, (units, st) in runs.items():
            T, uniq, cnt, _flags = units
            assert not overflowed(units).any(), (bits, np.argwhere(overflowed(units)).tolist())
            assert st.n_fallback_units == 0 and st.n_requeried == 0, (bits, st.n_fallback_units, st.n_requeried)
            for q, (_name, mults) in enumerate(DUPS):
                assert T[q, 0] == n * L and uniq[q, 0] == n * L - sum(mults) + len(mults), (bits, q, uniq[q, 0])
                assert cnt[q, 0] == uniq[q, 0], (bits, q, "a unit under keep_all offers every tweet")
            for q in (q_thread, q_waves):
                assert T[q, 0] == n * L and uniq[q, 0] == n * L - 2 and cnt[q, 0] == uniq[q, 0], (bits, q, uniq[q, 0], cnt[q, 0])
            assert T[q_all, 0] == 120 and uniq[q_all, 0] == 60 and cnt[q_all, 0] == 60, (bits, uniq[q_all, 0], cnt[q_all, 0])
            assert T[q_64, 0] == 128 and uniq[q_64, 0] == 65 and cnt[q_64, 0] == 65, (bits, uniq[q_64, 0], cnt[q_64, 0])
            n_false = np.array([len(c) for c in cores])
            assert (T[q_false] == n_false).all() and (uniq[q_false] == n_false).all() and (cnt[q_false] == n_false).all(), (bits, uniq[q_false], cnt[q_false])
    index.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. dead slots
def test_window_and_source_leave_dead_slots(pkg, oracle, lib, monkeypatch):
    """A 12 h window removes the older half of every unit's postings, spread over all its slots, and each query's source
    tweet is one of its young postings: unit 0 of each query loses that one too."""
    P, n = 4, 50
    lo12, _hi = sd.window(12)
    b = Builder(lib, P, 700)
    sizes = ((144, 144, 144, 144), (1536, 1300, 700, 129))
    for s in sizes:
        b.query(counts_for(s, n), np.exp(b.rng.normal(0.0, 0.5, n)), plant=planter(b, [2, 3]))
    csr, emb = b.finish()
    offs = emb[0]
    lists = {cid: ids for cid, ids in b.lists}
    sources, young = [], []
    for q in range(2):
        ids = np.concatenate([lists[c] for c in emb[1][offs[q]:offs[q + 1]]])
        y = np.unique(ids[ids >= lo12])
        part = sd.partitions(lib, y, P)
        assert 0.3 < len(y) / len(np.unique(ids)) < 0.7
        sources.append(int(y[part == 0][0]))
        young.append(np.bincount(part, minlength=P))
    index = pkg.ClusterTweetIndex(*csr, n_partitions=P)
    for alg in (2, 4):
        runs = both_offsets(pkg, oracle, monkeypatch, index, csr, emb, [sd.Cfg(40, 20000, 12, alg)] * 2, ("window", alg), sources=sources)
        for bits, (units, st) in runs.items():
            T, uniq, _cnt, _flags = units
            assert not overflowed(units).any(), bits
            assert np.array_equal(T, np.array(sizes)), (bits, T)
            for q in range(2):
                assert np.array_equal(uniq[q], young[q] - np.array([1, 0, 0, 0])), (bits, q, uniq[q], young[q])
            assert st.n_fallback_units == 4 * st.n_requeried, (bits, st.n_fallback_units, st.n_requeried)
    index.close()
