"""The duplicate phase of unit_fast_kernel (3b, "resolve flagged ids") on hand-built units: match lists of 2 ... 66 entries
whose groups' postings sit in chosen threads and waves of the workgroup, and filters that act on a group.

A case is ONE query of a batch; a batch is one tiny index per geometry.  Every query's clusters are its own, and one of
its (query, partition) units -- the "planted" unit -- holds the tweets that occur in two or three of its clusters.  Every
query of every batch is compared with the oracle bit for bit (ids, score bits, count, map size); between run() and
finish() the test also asserts that no unit overflowed and that the unit kernel's count of distinct live tweets
(unit_unique = live postings - folded ones) is the host model's, and afterwards that no query was re-run: the path under
test is the one that answered.

Where a posting sits.  A unit's postings are numbered cluster by cluster in scan order (ascending cluster id), inside a
cluster in list order (score descending) restricted to the partition; posting i belongs to thread i mod WG, slot
i div WG, wave (i mod WG) div 64.  The designs place every group's postings by that rule and assert the placement from
the computed indices: all of a group in one wave; in different waves with the representative (the posting of the lowest
cluster) outside wave 0; two postings of a group in one thread.

Which path.  nm (asserted from the host model sd.match_list, with `clean`) = 2 per pair + 3 per triple.  Lists up to
SHORT_NM = 12 entries are settled by every wave for itself, 13 ... 64 are sorted in wave 0's registers, longer ones
(geometries with a 128-entry list) compared pairwise by one thread per entry.

About two of the filters.  The age window looks at the tweet id, so it removes ALL postings of a tweet or none: the
"window" case removes a duplicated tweet whole (no group, not counted), and the posting-level filter that leaves ONE
posting of a pair is maxTopTweetsPerCluster (the "m_cut" case: no group is left and the map counts the tweet once).
And a group's summed score is never below BOTH of its postings' single scores under any of the algorithms (it is a
mediant of them or more): the "min_score" case puts minScore between the sum and the better single posting's score, so
a fold that failed would let that posting through."""
import dataclasses
from typing import Dict, List, Optional, Tuple

import numpy as np
import pytest

import _sann_design as sd

pytestmark = pytest.mark.gpu

M_ALL = 20000
K = 24
SHORT_NM = 12  # sann_fast.hip
RECUT_M = 12   # maxTopTweetsPerCluster of the "recut" case
# geometry -> postings per cluster of the planted unit (sum <= capacity; more than one slot per thread).  Clusters 0 and 1
# carry the weight, the others are light (their groups stay out of the top k).  No sub-list is longer than
# sd.SUBLIST_MAX: a cosine unit keeps ALL postings of the cluster its cut falls into, and the survivor list holds 160.
SUBLISTS = {
    # (the last cluster's list is the longest: the "m_cut" case cuts its last posting alone)
    256: [30, 28, 32, 26, 30, 30, 28, 34],             # <64, 4>: one wave, 238 postings, slots 0 ... 3
    # (and the heavy clusters 0 and 1 reach into every wave)
    512: [90, 80, 40, 40, 50, 50, 56, 92],             # <128, 4>: two waves, 498 postings
    1536: [98, 96, 90, 84, 88, 80, 92, 86, 78, 90, 84, 88, 82, 94, 80, 100],  # <256, 6>: four waves, 1410 postings, slots 0 ... 5
}
assert all(max(v) <= sd.SUBLIST_MAX and max(v[:-1]) < v[-1] for v in SUBLISTS.values())


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


@dataclasses.dataclass
class Spec:
    name: str
    groups: List[List[int]]            # flat posting indices of the planted unit, one list per duplicated tweet
    nm: Optional[int] = None           # match-list entries expected (None: not asserted -- the collision case)
    hours: int = 24
    weights: Optional[List[float]] = None
    source_group: Optional[int] = None  # the query's source tweet is this group's tweet
    old_groups: Tuple[int, ...] = ()    # groups whose tweet is older than the 12 h window
    m_cut: bool = False                 # the last posting of the last cluster's list is cut by maxTopTweetsPerCluster
    min_score_group: Optional[int] = None
    withholds: bool = False             # the planted unit must offer fewer candidates than it has live tweets
    collide: bool = False               # plant ids that flag the unit by Bloom collisions only
    m_top: Optional[int] = None         # P = 1: maxTopTweetsPerCluster; the unit then holds m_top postings per cluster
    placement: Dict[int, str] = dataclasses.field(default_factory=dict)  # group -> one_wave / rep_not_wave0 / same_thread


def geometry(cap):
    return sd.GEOMETRY[cap]


class Unit:
    """Index arithmetic of the planted unit of a geometry."""

    def __init__(self, cap):
        self.cap = cap
        self.WG, self.U = geometry(cap)
        self.L = SUBLISTS[cap]
        self.n_cl = len(self.L)
        self.pre = np.concatenate([[0], np.cumsum(self.L)]).astype(int)
        assert self.pre[-1] <= cap and self.pre[-1] > self.WG
        self.used = set()

    def cluster_of(self, i):
        return int(np.searchsorted(self.pre, i, side="right") - 1)

    def find(self, c, wave=None, thread=None, slot=None, last=False):
        """An unused posting of cluster c in the wanted wave / thread / slot (`last`: searching from the cluster's end)."""
        rng_ = range(self.pre[c], self.pre[c + 1])
        for i in (reversed(rng_) if last else rng_):
            if i in self.used:
                continue
            if wave is not None and (i % self.WG) // 64 != wave:
                continue
            if thread is not None and i % self.WG != thread:
                continue
            if slot is not None and i // self.WG != slot:
                continue
            self.used.add(i)
            return i
        raise AssertionError(f"no posting of cluster {c} with wave {wave} thread {thread} slot {slot}")

    def waves_of(self, c):
        return sorted({(i % self.WG) // 64 for i in range(self.pre[c], self.pre[c + 1])})

    def place(self, i):
        return i % self.WG, i // self.WG, (i % self.WG) // 64  # thread, slot, wave


def check_placement(un: Unit, group: List[int], kind: str):
    cl = [un.cluster_of(i) for i in group]
    assert len(set(cl)) == len(cl), "a tweet occurs once per cluster"
    thr, slot, wave = zip(*[un.place(i) for i in group])
    rep = int(np.argmin(cl))
    if kind == "one_wave":
        assert len(set(wave)) == 1, (group, wave)
    elif kind == "rep_not_wave0":
        assert len(set(wave)) > 1 and wave[rep] != 0, (group, wave)
    elif kind == "same_thread":
        assert any(thr[a] == thr[b] and slot[a] != slot[b] for a in range(len(group)) for b in range(a)), (group, thr, slot)
    else:
        raise AssertionError(kind)


def light_pairs(un: Unit, n_pairs: int, n_triples: int = 0) -> List[List[int]]:
    """Groups in the light clusters 2 ... 7, wherever there is room."""
    out = []
    for g in range(n_pairs + n_triples):
        cs = [2 + (g + t * 2) % 6 for t in range(3 if g >= n_pairs else 2)]
        out.append([un.find(c) for c in sorted(cs)])
    return out


def specs_for(cap: int, P: int = 4) -> Tuple[Unit, List[Spec]]:
    """The batch of a geometry.  Group 0 of most queries joins the heavy clusters 0 and 1: its tweet is among the
    query's best, so the answers themselves depend on the fold and on the representative's sums."""
    un = Unit(cap)
    WG = un.WG
    n_waves = WG // 64
    hi = max(set(un.waves_of(0)) & set(un.waves_of(1)))        # a wave both heavy clusters reach (not wave 0 where there are waves)
    other = [w_ for w_ in un.waves_of(1) if w_ != hi][:1]      # and another one of cluster 1
    assert n_waves == 1 or (hi != 0 and other)
    other = other[0] if other else 0
    S: List[Spec] = []

    def fresh():
        un.used = set()

    # nm = 2: a pair in one wave (the last one)
    fresh()
    S.append(Spec("nm2", [[un.find(0, wave=hi), un.find(1, wave=hi)]], 2, placement={0: "one_wave"}))
    # nm = 3: one tweet in three clusters; in different waves with the representative outside wave 0 where there are waves
    fresh()
    if n_waves > 1:
        S.append(Spec("nm3", [[un.find(0, wave=hi), un.find(1, wave=other), un.find(2)]], 3, placement={0: "rep_not_wave0"}))
    else:
        S.append(Spec("nm3", [[un.find(0), un.find(1), un.find(2)]], 3, placement={0: "one_wave"}))
    # nm = 4: two pairs, one of them in ONE thread (slots u and u')
    fresh()
    a = un.find(0, slot=0)
    b = un.find(un.cluster_of(a % WG + WG), thread=a % WG)
    S.append(Spec("nm4", [[a, b]] + light_pairs(un, 1), 4, placement={0: "same_thread"}))
    # nm = 5: pair + triple
    fresh()
    g0 = [un.find(0, wave=hi), un.find(1, wave=other)] if n_waves > 1 else [un.find(0), un.find(1)]
    S.append(Spec("nm5", [g0] + light_pairs(un, 0, 1), 5, placement={0: "rep_not_wave0"} if n_waves > 1 else {}))
    # the bound and one above it; a sorted-path size; (128-entry lists only) a long pairwise size
    for nm in (SHORT_NM, SHORT_NM + 1, 40) + ((66,) if sd.mcap(cap) > 64 else ()):
        fresh()
        g0 = [un.find(0, wave=hi), un.find(1, wave=other)] if n_waves > 1 else [un.find(0), un.find(1)]
        triples = nm % 2
        pairs = (nm - 2 - 3 * triples) // 2
        S.append(Spec(f"nm{nm}", [g0] + light_pairs(un, pairs, triples), nm, placement={0: "rep_not_wave0"} if n_waves > 1 else {}))
    # ---- filters acting on groups ------------------------------------------------------------------------------------
    # a 12 h window that removes a duplicated tweet whole; a second duplicated tweet stays
    fresh()
    S.append(Spec("window", [[un.find(0), un.find(1)], [un.find(0), un.find(2)]], 2, hours=12, old_groups=(0,)))
    # maxTopTweetsPerCluster cuts ONE posting of a pair (the last of the last cluster's list): no group is left
    fresh()
    S.append(Spec("m_cut", [[un.find(0), un.find(un.n_cl - 1, last=True)]], 0, m_cut=True))
    # the excluded source tweet is a duplicated tweet (another pair keeps the unit on the path)
    fresh()
    S.append(Spec("source", [[un.find(0), un.find(1)], [un.find(0), un.find(1)]], 2, source_group=0))
    # the summed score falls under minScore, the heavy posting alone would pass: heavy cluster 0's LOWEST score with light
    # cluster 3's HIGHEST
    fresh()
    S.append(Spec("min_score", [[un.find(0, last=True), un.find(3)], [un.find(0), un.find(1)]], 4, min_score_group=0))
    # ---- a representative on each side of the cut (cosine: the cluster-level cut lies at cluster 0's key) ---------------
    # group 0: clusters 1 and 2 (0.93 and 0.6, both under the cut), equal ranks: the summed key is above it.
    # group 1: cluster 0's lowest score with light cluster 3's highest: the representative sits in a cluster above the
    # cut, its summed key far below.
    fresh()
    S.append(Spec("cut_sides", [[un.find(1), un.find(2)], [un.find(0, last=True), un.find(3)]], 4, withholds=True,
                  weights=[1.0, 0.93, 0.6] + [0.05] * (un.n_cl - 3)))
    # ---- P = 1, the unit is the query: the cluster-level cut counts kl = k = 24 postings, the 12 best of clusters 0 and 1
    # (maxTopTweetsPerCluster = 12); five tweets are in both, so 19 candidates are left above the cut.  Only the re-cut
    # (survivors + folded >= kl) lets the unit offer k: without it the query cannot be proven and is re-run.
    if P == 1:
        S.append(Spec("recut", [[2 * g + 1, RECUT_M + 2 * g] for g in range(5)], 10, m_top=RECUT_M, withholds=True))
    # ---- flagged by hash collisions only ------------------------------------------------------------------------------
    S.append(Spec("collide", [], None, collide=True))
    return un, S


def locate(un: Unit, S: Spec, i: int) -> Tuple[int, int]:
    """(cluster, rank in the cluster's sub-list) of posting i of the planted unit."""
    if S.m_top is not None:
        return i // S.m_top, i % S.m_top
    c = un.cluster_of(i)
    return c, i - int(un.pre[c])


def base_score(L: int, j: int) -> float:
    """Score of rank j of a sub-list of L: 0.5 down to 0.02, geometric (the jitter on top keeps the order)."""
    return 0.5 * (0.04 ** (j / max(L - 1, 1)))


def colliding_ids(lib, cap: int, P: int, p0: int, avoid: set, n_sets: int = 6) -> List[List[int]]:
    """Sets [i, o1, o2, ...] of distinct pool ids of partition p0, all of one Bloom word, where the others' bits cover
    all four bits of i: when i arrives after them it is flagged although no id occurs twice."""
    BW = 8 if cap <= 512 else 9 if cap <= 1024 else 11
    ids = sd.streams(lib, P)[p0]
    ids = ids[~np.isin(ids, np.fromiter(avoid, np.int64, len(avoid)))] if avoid else ids
    hv = sd.table_hash(ids, 20 + BW)
    word, bits = (hv >> np.uint64(20)).astype(np.int64), sd.bloom_bits(hv)
    order = np.argsort(word, kind="stable")
    out = []
    start = 0
    w_sorted = word[order]
    while start < len(order) and len(out) < n_sets:
        end = start
        while end < len(order) and w_sorted[end] == w_sorted[start]:
            end += 1
        members = order[start:end]
        start = end
        for i in members:
            need = int(bits[i])
            cover = []
            for o in members:
                if o != i and int(bits[o]) & need:
                    cover.append(o)
                    need &= ~int(bits[o])
                if not need:
                    break
            if not need and len(cover) <= 4:
                out.append([int(ids[i])] + [int(ids[o]) for o in cover])
                break
    assert len(out) == n_sets, "the id pool holds too few colliding sets"
    return out


def build(lib, cap: int, P: int, seed: int = 0, skips: Optional[Dict[int, int]] = None):
    """-> (Design, Unit, specs, p0 per query, source per query, planted tweet per (query, group))."""
    un, specs = specs_for(cap, P)
    rng = np.random.default_rng([cap, P, seed, 8])
    st = sd.streams(lib, P)
    lo12, _ = sd.window(12)
    cur = np.full(P, 400 * seed, np.int64)  # (another seed also means other tweets)
    lists, queries, embs = {}, [], []
    p0s, sources, planted, min_scores = [], [], {}, []
    for q, S in enumerate(specs):
        p0 = q % P
        p0s.append(p0)
        cur[p0] += 97 * (skips or {}).get(q, 0)  # (other tweets for this query's planted unit)
        w = np.array(S.weights if S.weights else [1.0, 0.93] + list(0.05 * np.exp(rng.normal(0.0, 0.3, un.n_cl - 2))))
        sub_ids = [[None] * P for _ in range(un.n_cl)]
        for p in range(P):
            for c in range(un.n_cl):
                n = un.L[c]
                a = st[p][cur[p]:cur[p] + n].copy()
                assert len(a) == n, "the id pool is too small for this design"
                cur[p] += n
                sub_ids[c][p] = a
        # old tweets for the window case: ids under the 12 h bound, from the far end of the stream
        old = st[p0][st[p0] < lo12][::-1]
        assert len(old) > 8
        for g, grp in enumerate(S.groups):
            c0, j0 = locate(un, S, grp[0])
            x = int(old[g]) if g in S.old_groups else int(sub_ids[c0][p0][j0])
            if S.hours == 12 and g not in S.old_groups:  # a tweet the window keeps
                x = int(st[p0][st[p0] >= lo12][-1 - g])
            for i in grp:
                c, j = locate(un, S, i)
                sub_ids[c][p0][j] = x
            planted[(q, g)] = x
        if S.collide:
            flat = [t for s_ in colliding_ids(lib, cap, P, p0, set(np.concatenate([a for row in sub_ids for a in row]).tolist())) for t in s_]
            assert len(set(flat)) == len(flat)
            for n_, t in enumerate(flat):  # anywhere in the unit, one per posting
                c = n_ % un.n_cl
                sub_ids[c][p0][n_ // un.n_cl] = t
        for c in range(un.n_cl):
            ids_c, sc_c = [], []
            for p in range(P):
                n = len(sub_ids[c][p])
                ids_c.append(sub_ids[c][p])
                sc_c.append(np.array([base_score(n, j) for j in range(n)]) * (1.0 + 1e-3 * rng.random(n)))
            ids_c, sc_c = np.concatenate(ids_c), np.concatenate(sc_c)
            if S.m_cut and c == un.n_cl - 1:  # the planted unit's last posting of this list becomes the list's last: cut by M
                at = int(sum(len(sub_ids[c][p]) for p in range(p0)) + len(sub_ids[c][p0]) - 1)
                sc_c[at] = 0.5 * sc_c.min()
            lists[1000 * q + 1 + c] = (ids_c, sc_c)
        M = M_ALL
        if S.m_top is not None:
            assert P == 1 and all(n >= S.m_top for n in un.L)  # (one partition: a list's rank is the sub-list's)
            M = S.m_top
        if S.m_cut:
            M = len(lists[1000 * q + un.n_cl][0]) - 1
            assert all(len(lists[1000 * q + 1 + c][0]) <= M for c in range(un.n_cl - 1)), "only the last list may be cut"
        embs.append((1000 * q + 1 + np.arange(un.n_cl), w))
        queries.append(sd.Query(S.name, un.n_cl, M, None, dup_unit=p0, nm=S.nm or 0))
        sources.append(planted[(q, S.source_group)] if S.source_group is not None else None)
    # (as tests/test_sann_load_grouping_gpu.py builds its designs)
    cids = sorted(lists)
    offs, tid, sc = [0], [], []
    for c in cids:
        ids_c, s_c = lists[c]
        order = np.lexsort((ids_c, -s_c))
        tid.append(ids_c[order])
        sc.append(s_c[order])
        offs.append(offs[-1] + len(ids_c))
    eo = np.zeros(len(embs) + 1, np.int64)
    eo[1:] = np.cumsum([len(e[0]) for e in embs])
    d = sd.Design(cap, P, False, queries, np.array(cids, np.int32), np.array(offs, np.int64), np.concatenate(tid), np.concatenate(sc), eo,
                  np.concatenate([np.asarray(e[0], np.int32) for e in embs]), np.concatenate([np.asarray(e[1], np.float64) for e in embs]))
    assert len(np.unique(d.scores)) == len(d.scores), "scores must be distinct"
    assert len(d.tweet_ids) < 300_000
    return d, un, specs, p0s, sources, planted


_BUILT: Dict[Tuple[int, int], tuple] = {}
# A planted unit in which a Bloom collision could flag a posting of another id (match_list's `clean` is False) draws
# other tweets: (seed of the design, {query: strides of 97 ids skipped in its planted partition's stream}).  The 256- and
# 512-word filters of the small geometries collide often; check_design asserts the outcome.
DRAWS: Dict[Tuple[int, int], Tuple[int, Dict[int, int]]] = {(512, 4): (0, {5: 1, 7: 2, 8: 2}), (1536, 4): (0, {9: 6}), (1536, 1): (0, {5: 4})}


def built(lib, cap, P):
    if (cap, P) not in _BUILT:
        _BUILT[(cap, P)] = build(lib, cap, P, *DRAWS.get((cap, P), (0, None)))
    return _BUILT[(cap, P)]


def group_postings(d, un, S, q, p0, lib):
    """Per group: [(cluster sequence, score)] of its postings in the planted unit, from the design's CSR arrays."""
    out = []
    cl, _w = d.emb(q)
    for grp in S.groups:
        rows = []
        for i in grp:
            c, j = locate(un, S, i)
            r = int(np.searchsorted(d.cluster_ids, cl[c]))
            a, b = int(d.list_offsets[r]), int(d.list_offsets[r + 1])
            ids, sc = d.tweet_ids[a:b], d.scores[a:b]
            sub = np.nonzero(sd.partitions(lib, ids, d.P) == p0)[0]
            rows.append((c, float(sc[sub[j]]), int(ids[sub[j]])))
        out.append(rows)
    return out


def check_design(lib, d, un, specs, p0s, sources, planted):
    """What the cases claim, from the design itself: placement, nm and `clean`, the planted ids, the cut sides."""
    T = sd.unit_T(lib, d)
    beats = []  # per query: group 0's cosine is above every single posting's (the heaviest cluster's weight)
    for q, S in enumerate(specs):
        p0 = p0s[q]
        assert T[q, p0] == (un.n_cl * S.m_top if S.m_top is not None else un.pre[-1] - (1 if S.m_cut else 0)), (S.name, T[q].tolist())
        assert T[q].max() <= d.cap, (S.name, T[q].tolist())
        if S.m_top is not None:  # the two best clusters' m_top postings are exactly kl, the unit is the query and withholds
            kl = sd.unit_kl(K, d.P)
            assert d.P == 1 and 2 * S.m_top == kl == K and T[q, p0] - len(S.groups) > min(sd.FAST_SCAP, kl + kl // 2 + 16)
        for g, kind in S.placement.items():
            check_placement(un, S.groups[g], kind)
        rows = group_postings(d, un, S, q, p0, lib)
        for g, r in enumerate(rows):  # the postings at the computed indices ARE the planted tweet's
            if not (S.m_cut and g == 0):
                assert all(t == planted[(q, g)] for _c, _s, t in r), (S.name, g)
        if S.nm is not None:
            nm, clean = sd.match_list(lib, d, q, p0, S.hours, sources[q])
            assert (nm, clean) == (S.nm, True), (S.name, nm, clean)
        if S.collide:
            ids = sd.scanned_postings(d, q)[0]
            assert len(np.unique(ids)) == len(ids), "no id of the collision case occurs twice"
            assert not sd.match_list(lib, d, q, p0)[1], "the collision case must be able to flag"
        cl, w = d.emb(q)
        l2 = float(np.sqrt((w * w).sum()))
        cos = lambda r: sum(s * w[c] for c, s, _t in r) / np.sqrt(sum(s * s for _c, s, _t in r)) / l2
        if S.name == "cut_sides":
            cut = w[0] / l2  # the unit holds more than unit_kl postings of cluster 0: the cluster-level cut is its key
            assert un.L[0] >= sd.unit_kl(K, d.P)
            assert cos(rows[0]) > cut * 1.01 and max(w[c] for c, _s, _t in rows[0]) < w[0]
            assert cos(rows[1]) < cut * 0.5 and min(c for c, _s, _t in rows[1]) == 0
        if S.min_score_group is not None:
            r = rows[S.min_score_group]
            assert cos(r) < 0.5 * w[0] / l2 < w[0] / l2
        filtered = S.old_groups or S.m_cut or S.source_group is not None or S.min_score_group is not None
        beats.append(bool(rows) and not filtered and cos(rows[0]) > 1.001 * w.max() / l2)
    assert sum(beats) >= 6, beats
    return beats


def min_score_of(d, S, q, alg):
    """The "min_score" case under cosine: halfway under the heavy posting's single score (see check_design)."""
    if S.min_score_group is None or alg != 2:
        return 0.0
    _cl, w = d.emb(q)
    return float(0.5 * w[0] / np.sqrt((w * w).sum()))


def _batch(pkg, d, index, cfgs, sources, alg):
    pc = [pkg.SimClustersANNConfig(maxNumResults=c.maxNumResults, minScore=c.minScore, maxTopTweetsPerCluster=c.maxTopTweetsPerCluster,
                                   maxScanClusters=c.maxScanClusters, maxTweetCandidateAgeHours=c.maxTweetCandidateAgeHours,
                                   annAlgorithm=pkg.ScoringAlgorithm(alg)) for c in cfgs]
    src = np.array([0 if s is None else s for s in sources], np.int64)
    has = np.array([0 if s is None else 1 for s in sources], np.uint8)
    return pkg.QueryBatch(index, d.emb_offsets, d.emb_cids, d.emb_scs, pc, now_ms=sd.NOW_MS, source_tweet_ids=src, has_source_tweet=has)


def _same(ids, scores, counts, msz, q, o_ids, o_sc, o_msz, tag):
    assert counts[q] == len(o_ids), (tag, q, counts[q], len(o_ids))
    assert msz[q] == o_msz, (tag, q, msz[q], o_msz)
    assert np.array_equal(ids[q, :counts[q]], o_ids), (tag, q, "id order differs")
    assert np.array_equal(scores[q, :counts[q]].view(np.int64), np.asarray(o_sc).view(np.int64)), (tag, q, "scores differ")


_EXPECTED: Dict[tuple, list] = {}


def expected(oracle, d, key, cfgs, sources):
    """The oracle's answers of a (design, algorithm): computed once, shared, never modified."""
    if key not in _EXPECTED:
        out = []
        for q in range(d.nq):
            cl, w = d.emb(q)
            out.append(oracle.sann_query(cl, w, sources[q], cfgs[q], sd.NOW_MS, d.cluster_ids, d.list_offsets, d.tweet_ids, d.scores))
        _EXPECTED[key] = out
    return _EXPECTED[key]


def run_fast_path(qb, d, specs, p0s, live, tag):
    """run(); the fast path's own bookkeeping; finish().  -> (ids, scores, counts, map sizes)."""
    qb.run()
    _uT, uniq, cnt, flags = qb.unit_arrays()
    reasons = qb.overflow_reasons()
    assert not (flags & sd.UNIT_OVERFLOW).any() and not reasons.any(), (tag, "overflow", reasons.tolist())
    assert np.array_equal(uniq, live), (tag, "unit_unique", np.argwhere(uniq != live)[:8].tolist())
    for q, S in enumerate(specs):
        if S.withholds:
            assert cnt[q, p0s[q]] < uniq[q, p0s[q]], (tag, S.name, "the unit offered everything")
    qb.finish()
    out = qb.results()
    st = qb.stats()
    assert st.n_requeried == 0 and st.n_fallback_units == 0, (tag, st.n_requeried, st.n_fallback_units)
    return out


def configs(d, specs, alg, k=K):
    return [sd.Cfg(k, Q.M, S.hours, alg, minScore=min_score_of(d, S, q, alg)) for q, (Q, S) in enumerate(zip(d.queries, specs))]


CASES = [(256, 4, (2,)), (512, 4, (2,)), (1536, 4, (2, 3, 1)), (1536, 1, (2,))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"cap{c[0]}-P{c[1]}")
def test_dup_settle(pkg, oracle, lib, monkeypatch, case):
    """Capacity 256 (<64, 4>: the wave is the workgroup), 512 (<128, 4>) and 1536 (<256, 6>) at P = 4; 1536 at P = 1, where
    the unit is the query and the re-cut condition `survivors + folded >= kl` decides whether it offers k at all."""
    cap, P, algs = case
    monkeypatch.setenv("SANN_UNIT_CAP", str(cap))
    d, un, specs, p0s, sources, planted = built(lib, cap, P)
    print(f"unit_fast_kernel<{un.WG}, {un.U}, 64>, P = {P}: " + ", ".join(f"{S.name}({S.nm})" for S in specs))
    beats = check_design(lib, d, un, specs, p0s, sources, planted)
    index = pkg.ClusterTweetIndex(d.cluster_ids, d.list_offsets, d.tweet_ids, d.scores, n_partitions=P)
    live = np.zeros((d.nq, P), np.int64)
    for q, S in enumerate(specs):  # (unit_live takes one window for the batch: query by query here)
        live[q] = sd.unit_live(lib, d, S.hours, sources)[q]
    for alg in algs:
        tag = (cap, P, alg)
        cfgs = configs(d, specs, alg)
        want = expected(oracle, d, (cap, P, alg), cfgs, sources)
        qb = _batch(pkg, d, index, cfgs, sources, alg)
        ids, scores, counts, msz = run_fast_path(qb, d, specs, p0s, live, tag)
        qb.close()
        for q in range(d.nq):
            _same(ids, scores, counts, msz, q, *want[q], tag + (specs[q].name,))
        # the answers depend on the fold: a duplicated tweet whose cosine beats every single posting's is among them
        for q, S in enumerate(specs):
            if alg == 2 and beats[q]:
                assert planted[(q, 0)] in ids[q, :counts[q]].tolist(), (tag, S.name)
    index.close()


def test_dup_settle_offline_norms(pkg, oracle, lib, monkeypatch):
    """The offline forms on the 1536 geometry: a representative's normaliser is ONE norm per tweet (s_Mnrm), not a sum."""
    cap, P = 1536, 4
    monkeypatch.setenv("SANN_UNIT_CAP", str(cap))
    d, un, specs, p0s, _sources, _planted = built(lib, cap, P)
    d = dataclasses.replace(d, norms=None)
    d.norms = sd.full_norms(d)
    assert (d.norms > 0.0).all()
    none = [None] * d.nq
    live = sd.unit_live(lib, d, offline=True)
    for q, S in enumerate(specs):
        if S.nm is not None:  # (no window and no source tweet offline: those two cases keep both of their pairs)
            nm = sum(len(g) for g in S.groups) if S.old_groups or S.source_group is not None else S.nm
            assert sd.match_list(lib, d, q, p0s[q], offline=True) == (nm, True), S.name
    rows = sd.sql_rows(oracle, d)
    index = pkg.ClusterTweetIndex(d.cluster_ids, d.list_offsets, d.tweet_ids, d.scores, n_partitions=P, tweet_norms=d.norms)
    for alg in (5, 6):
        tag = ("offline", alg)
        cfgs = [sd.Cfg(K, Q.M, 175200, alg, minScore=-1e300) for Q in d.queries]
        qb = _batch(pkg, d, index, cfgs, none, alg)
        ids, scores, counts, msz = run_fast_path(qb, d, [dataclasses.replace(S, withholds=False) for S in specs], p0s, live, tag)
        qb.close()
        col = 3 if alg == 5 else 2
        for q in range(d.nq):
            want = sorted(rows[q], key=lambda r: (-r[col], r[0]))[:K]
            _same(ids, scores, counts, msz, q, np.array([r[0] for r in want], np.int64), np.array([r[col] for r in want]), len(rows[q]),
                  tag + (specs[q].name,))
    index.close()


def test_dup_settle_deterministic(pkg, lib, monkeypatch):
    """Twenty runs of the four-wave batch in one process: the four output arrays of every run equal the first run's."""
    cap, P = 1536, 4
    monkeypatch.setenv("SANN_UNIT_CAP", str(cap))
    d, _un, specs, _p0s, sources, _planted = built(lib, cap, P)
    index = pkg.ClusterTweetIndex(d.cluster_ids, d.list_offsets, d.tweet_ids, d.scores, n_partitions=P)
    qb = _batch(pkg, d, index, configs(d, specs, 2), sources, 2)
    first = None
    for run in range(20):
        qb.run()
        qb.finish()
        out = qb.results()
        if first is None:
            first = [a.copy() for a in out]
        for name, a, b in zip(("ids", "scores", "counts", "map sizes"), first, out):
            assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b), (run, name)
    qb.close()
    index.close()
