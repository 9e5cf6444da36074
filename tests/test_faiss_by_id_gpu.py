"""include/faiss_by_id.h on the device.  The contract under test: the triples of a found seed are, byte for byte (ids,
distance bits, counts), the row the plain search returns for ann_store_get(store, seed) -- for every index kind, metric,
nprobe and ht.  Shapes are the smallest at which the new kernels can go wrong: 2,000 rows in 8 lists, a store of 2,500
keys that is a superset of the index's rows; d = 16 (one 16-byte piece per lane of the gather and idle lanes), 48 (an odd
piece count), 512 (the widest row); OPQ d_in = 40 (no multiple of 16) -> d_out = 32."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _ivfhq_ref as hqref
import _polysemous_ref as polyref

pytestmark = pytest.mark.gpu

EINVAL = 1
N, N_STORE, NLIST, NITER = 2000, 2500, 8, 2
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SENTINEL_I, SENTINEL_F = 0x5A5A5A5A5A5A5A5A, np.float32(-12345.5)
METRICS = ["L2", "InnerProduct", "Cosine"]


@pytest.fixture(scope="module")
def fb(pkg):
    return importlib.import_module(pkg.__name__ + ".faiss_by_id")


@pytest.fixture(scope="module")
def sq(pkg):
    return importlib.import_module(pkg.__name__ + ".scalar_quantizer")


@pytest.fixture(scope="module")
def hq(pkg):
    return importlib.import_module(pkg.__name__ + ".hnsw_quantizer")


def _metric(pkg, name):
    return getattr(pkg.dense_ann.DistanceMetric, name)


def _keys(rng, n):
    """n unique int64 keys: negative values, values above 2^53 (where a double would merge neighbours) and the ends of the range."""
    special = [I64_MIN, I64_MIN + 1, -1, 0, 1, (1 << 53) + 1, (1 << 53) + 3, -(1 << 53) - 1, I64_MAX - 1, I64_MAX]
    rest = np.unique(rng.integers(-(1 << 62), 1 << 62, 2 * n, dtype=np.int64))
    rest = rest[~np.isin(rest, special)]
    keys = np.concatenate([np.array(special, np.int64), rng.permutation(rest)[:n - len(special)]])
    return rng.permutation(keys)


ABSENT = np.array([I64_MIN + 2, I64_MAX - 2, (1 << 53) + 2, 5, -2], np.int64)  # neighbours of stored keys, not stored


def _data(seed, d):
    """rows [N_STORE][d] in 12 clusters, their keys; the first N rows (under their keys) go into the index."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((12, d)).astype(np.float32) * 2
    x = (centres[rng.integers(0, 12, N_STORE)] + rng.standard_normal((N_STORE, d)).astype(np.float32)).astype(np.float32)
    keys = _keys(rng, N_STORE)
    assert not np.isin(ABSENT, keys).any()
    return x, keys


def _seed_list(rng, keys, n_found, n_absent=0):
    """found (some repeated), absent and repeated seeds interleaved"""
    found = rng.choice(keys, n_found, replace=True)
    if n_found >= 4:
        found[3] = found[0]  # a seed given twice
    seeds = np.concatenate([found, rng.choice(ABSENT, n_absent, replace=True)]) if n_absent else found
    return np.ascontiguousarray(rng.permutation(seeds), np.int64)


class Case:
    """An index of one kind over the first N rows, the store over all rows, and the two calls to compare."""

    def __init__(self, pkg, fb, sq, kind, metric, d, seed=1):
        self.pkg, self.fb, self.kind, self.k_id = pkg, fb, kind, {"flat": 1, "pq": 2, "opq": 3, "sq8": 4}[kind]
        m = _metric(pkg, metric)
        self.x, self.keys = _data(seed, d)
        xi = self.x[:N]
        if kind == "flat":
            self.ix = pkg.ivf_ann.FaissIvfFlat.train(m, NLIST, xi, niter=NITER)
        elif kind == "sq8":
            self.ix = sq.FaissIvfSq8.train(m, NLIST, xi, niter=NITER)
        elif kind == "pq":
            self.ix = pkg.ivfpq_ann.FaissIvfPq.train(m, NLIST, 8, xi, niter=NITER)
        else:
            self.ix = pkg.opq_ann.FaissOpqIvfPq.train(m, NLIST, 8, 32, xi, niter=NITER)
        self.ix.add(xi, self.keys[:N])
        self.store = pkg.ann_by_id.EmbeddingStore.build(self.keys, self.x)
        self.prefix = {"flat": "ivf", "sq8": "ivfsq", "pq": "ivfpq", "opq": "opq"}[kind]
        self.has_ht = kind in ("pq", "opq")

    def handle(self):
        return self.ix._h

    def plain(self, q, k, nprobe, ht=0):
        if self.has_ht:
            return self.pkg.polysemous_ann.search_ht(self.ix, q, k, nprobe, ht)
        return self.ix.search(q, k, nprobe)

    def close(self):
        self.ix.close()
        self.store.close()


def _raw(case, seeds, k, nprobe, ht=0, cap=None, pad=64):
    """The C call with guarded buffers: (rc, seeds, ids, dist, counts, total); nothing may be written beyond out_total."""
    lib = case.fb._lib()
    n = len(seeds)
    cap = n * k if cap is None else cap
    o_seed = np.full(cap + pad, SENTINEL_I, np.int64); o_id = np.full(cap + pad, SENTINEL_I, np.int64)
    o_dist = np.full(cap + pad, SENTINEL_F, np.float32)
    cnt = np.full(n + pad, -99, np.int32)
    total = C.c_int64(-7)
    head = (case.handle(), case.store._h, n, seeds.ctypes.data, k, nprobe) + ((ht,) if case.has_ht else ())
    rc = getattr(lib, case.prefix + "_batch_query_by_id")(*head, o_seed.ctypes.data, o_id.ctypes.data, o_dist.ctypes.data, cap,
                                                         C.byref(total), cnt.ctypes.data)
    t = max(total.value, 0) if rc == 0 else 0
    assert np.all(o_seed[t:] == SENTINEL_I) and np.all(o_id[t:] == SENTINEL_I) and np.all(o_dist[t:] == SENTINEL_F), "written beyond out_total"
    assert np.all(cnt[n:] == -99)
    return rc, o_seed[:t], o_id[:t], o_dist[:t], cnt[:n], total.value


def _expected(case, seeds, k, nprobe, ht=0):
    """The host composition: ann_store_get -> the plain search over the found rows -> flatten."""
    rows, found = case.store.get(seeds)
    counts = np.full(len(seeds), -1, np.int32)
    if not found.any():
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32), counts
    ids, dist, cnt = case.plain(rows[found], k, nprobe, ht)
    counts[found] = cnt
    s = np.concatenate([np.full(c, sd, np.int64) for sd, c in zip(seeds[found].tolist(), cnt.tolist())])
    i = np.concatenate([ids[j, :c] for j, c in enumerate(cnt.tolist())])
    d = np.concatenate([dist[j, :c] for j, c in enumerate(cnt.tolist())])
    return s, i, d, counts


def _check(case, seeds, k, nprobe, ht=0, what=""):
    want = _expected(case, seeds, k, nprobe, ht)
    rc, s, i, d, c, total = _raw(case, seeds, k, nprobe, ht)
    assert rc == 0, case.fb._lib().ivf_by_id_last_error().decode()
    assert np.array_equal(c, want[3]), f"counts {what}"
    assert total == len(want[0]) == int(np.maximum(c, 0).sum())
    assert np.array_equal(s, want[0]), f"seeds {what}"
    assert np.array_equal(i, want[1]), f"ids {what}"
    assert np.array_equal(d.view(np.uint32), want[2].view(np.uint32)), f"distance bits {what}"
    return s, i, d, c


def _stats(case):
    v = [C.c_int64() for _ in range(5)]
    f = [C.c_float() for _ in range(3)]
    lib = case.fb._lib()
    assert lib.ivf_by_id_last_stats(case.k_id, case.handle(), *[C.byref(x) for x in v], *[C.byref(x) for x in f]) == 0
    names = ("found", "absent", "h2d_bytes", "d2h_bytes", "d2h_result_bytes", "resolve_gather_ms", "search_ms", "flatten_ms")
    return dict(zip(names, [x.value for x in v] + [x.value for x in f]))


# ---- 1. byte equality with the plain search over the fetched rows ---------------------------------------------------------
SHAPES = [(kind, d) for kind in ("flat", "sq8", "pq") for d in (16, 48, 512)] + [("opq", 40)]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind,d", SHAPES)
def test_by_id_is_the_plain_search_over_the_fetched_rows(pkg, fb, sq, kind, d, metric):
    case = Case(pkg, fb, sq, kind, metric, d, seed=3 + d)
    try:
        rng = np.random.default_rng(d)
        seeds = _seed_list(rng, case.keys, 37, 6)
        for k in (1, 10):
            for nprobe in (1, 8):
                s, i, dist, c = _check(case, seeds, k, nprobe, what=f"{kind} {metric} d={d} k={k} nprobe={nprobe}")
                st = _stats(case)
                assert st["found"] == 37 and st["absent"] == 6 and st["found"] + st["absent"] == len(seeds)
                assert st["d2h_result_bytes"] == 20 * len(s) + 4 * len(seeds)
                assert st["h2d_bytes"] == 8 * len(seeds), "the exhaustive quantizer uploads no control block"
                assert st["d2h_bytes"] > st["d2h_result_bytes"] + 8
        # the seed is not filtered out of its own answer: an index row under its own key is its own nearest (L2, nprobe = all)
        if metric == "L2" and kind in ("flat",):
            own = case.keys[:20]
            s, i, dist, c = _check(case, np.ascontiguousarray(own), 1, 8)
            assert np.array_equal(i, own)
    finally:
        case.close()


# ---- 2. seed lists ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flat16(pkg, fb, sq):
    case = Case(pkg, fb, sq, "flat", "L2", 16, seed=11)
    yield case
    case.close()


@pytest.fixture(scope="module")
def pq48(pkg, fb, sq):
    case = Case(pkg, fb, sq, "pq", "L2", 48, seed=12)
    yield case
    case.close()


@pytest.mark.parametrize("n_seeds", [0, 1, 31, 32, 33])
def test_seed_counts_around_the_scan_group(flat16, pq48, n_seeds):
    """n_seeds around the scan's 32-query group; with and without absent seeds in between."""
    rng = np.random.default_rng(100 + n_seeds)
    for case in (flat16, pq48):
        seeds = _seed_list(rng, case.keys, n_seeds)
        _check(case, seeds, 10, 3)
        if n_seeds:
            mixed = _seed_list(rng, case.keys, n_seeds, 5)
            _check(case, mixed, 10, 3)
            assert _stats(case)["found"] == n_seeds
    if n_seeds == 0:
        rc, s, i, d, c, total = _raw(flat16, np.zeros(0, np.int64), 10, 3)
        assert rc == 0 and total == 0
        st = _stats(flat16)
        assert st["found"] == 0 and st["absent"] == 0 and st["h2d_bytes"] == 0 and st["d2h_bytes"] == 0


@pytest.mark.parametrize("which", ["flat", "pq"])
def test_second_chunk_reads_its_own_positions(flat16, pq48, which):
    """4,130 found seeds: the second CHUNK of the search starts at pos + 4096, not at rows + 4096 * d."""
    case = flat16 if which == "flat" else pq48
    rng = np.random.default_rng(7)
    seeds = _seed_list(rng, case.keys, 4130, 9)
    s, i, d, c = _check(case, seeds, 2, 2)
    assert _stats(case)["found"] == 4130 and len(s) == 2 * 4130


def test_all_absent(flat16, pq48):
    for case in (flat16, pq48):
        seeds = np.ascontiguousarray(np.tile(ABSENT, 3))
        rc, s, i, d, c, total = _raw(case, seeds, 10, 4)
        assert rc == 0 and total == 0 and np.all(c == -1)
        st = _stats(case)
        assert st["found"] == 0 and st["absent"] == len(seeds) and st["search_ms"] == 0.0
        assert st["h2d_bytes"] == 8 * len(seeds) and st["d2h_result_bytes"] == 4 * len(seeds) and st["d2h_bytes"] == 4 * len(seeds) + 8


# ---- 3. short answers, cap ---------------------------------------------------------------------------------------------------
def test_short_answers_are_packed(flat16, pq48):
    """nprobe = 1 and k above the smallest list: counts differ from seed to seed and fall short of k; the triples are still
    packed seed after seed and nothing is written beyond out_total (_raw guards the buffers)."""
    for case in (flat16, pq48):
        k = 600
        assert case.ix.list_sizes().min() < k
        rng = np.random.default_rng(5)
        seeds = _seed_list(rng, case.keys, 40, 4)
        s, i, d, c = _check(case, seeds, k, 1)
        found = c[c >= 0]
        assert (found < k).any() and len(np.unique(found)) > 1 and len(s) == found.sum() < 40 * k
        at = 0
        for sd, m in zip(seeds.tolist(), c.tolist()):
            if m > 0:
                assert np.all(s[at:at + m] == sd) and np.all(np.diff(d[at:at + m]) >= 0)
                at += m


def test_cap(flat16, pq48):
    for case in (flat16, pq48):
        lib = case.fb._lib()
        rng = np.random.default_rng(6)
        seeds = _seed_list(rng, case.keys, 20, 5)
        q = case.x[:9]
        before = case.plain(q, 10, 3)
        want = _check(case, seeds, 10, 3)
        rc, s, i, d, c, total = _raw(case, seeds, 10, 3, cap=20 * 10)  # n_found * k, not n_seeds * k
        assert rc == 0 and np.array_equal(i, want[1]) and np.array_equal(d.view(np.uint32), want[2].view(np.uint32))
        rc, s, i, d, c, total = _raw(case, seeds, 10, 3, cap=20 * 10 - 1)
        assert rc == EINVAL and "cap" in lib.ivf_by_id_last_error().decode() and total == 0 and np.all(c == -99)
        after = case.plain(q, 10, 3)
        for a, b in zip(before, after):
            assert a.tobytes() == b.tobytes(), "a refused call leaves the index as it was"
        _check(case, seeds, 10, 3)


def test_store_of_another_dimension_is_refused(pkg, flat16):
    lib = flat16.fb._lib()
    other = pkg.ann_by_id.EmbeddingStore.build(np.arange(4), np.zeros((4, 32), np.float32))
    keep, flat16.store = flat16.store, other
    try:
        rc, *_ = _raw(flat16, np.arange(4, dtype=np.int64), 10, 3)
        assert rc == EINVAL and "dimension" in lib.ivf_by_id_last_error().decode()
    finally:
        flat16.store = keep
        other.close()


# ---- 4. ht ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [("pq", 48), ("opq", 40)])
def test_hamming_filter(pkg, fb, sq, kind, d):
    case = Case(pkg, fb, sq, kind, "L2", d, seed=21)
    try:
        rng = np.random.default_rng(8)
        seeds = _seed_list(rng, case.keys, 33, 3)
        rows, found = case.store.get(seeds)
        M, nprobe = 8, 2
        # on the host first: the Hamming filter over the exported codes keeps some rows of the probed lists and drops some
        case.plain(rows[found], 10, nprobe, 8 * M)
        probes, qcodes = case.ix.last_probes(), None
        nq32, np32 = C.c_int32(), C.c_int32()
        lib = pkg.polysemous_ann._lib()
        fn = getattr(lib, case.prefix + "_last_query_codes")
        assert fn(case.ix._h, C.byref(nq32), C.byref(np32), None) == 0
        qcodes = np.empty((nq32.value, np32.value, M), np.uint8)
        assert fn(case.ix._h, None, None, qcodes.ctypes.data) == 0
        codes, cells = case.ix.codes(), case.ix.assignment()[1]
        dists = np.concatenate([polyref.hamming(codes[cells == c], qcodes[qi, j]) for qi in range(len(probes))
                                for j, c in enumerate(probes[qi].tolist())])
        ht = int(np.median(dists)) + 1
        kept = int((dists < ht).sum())
        assert 0 < kept < len(dists), "the filter keeps some rows and drops some"
        s, i, dist, c = _check(case, seeds, 10, nprobe, ht)
        unfiltered = _check(case, seeds, 10, nprobe, 0)
        assert not np.array_equal(i, unfiltered[1]) or not np.array_equal(c, unfiltered[3]), "the filter changed the answer"
        _check(case, seeds, 10, nprobe, -3)  # ht <= 0: no filter
    finally:
        case.close()


# ---- 5. an HNSW coarse quantizer attached -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["flat", "pq"])
def test_hnsw_quantizer_is_inherited(pkg, fb, sq, hq, kind):
    case = Case(pkg, fb, sq, kind, "L2", 16, seed=31)
    try:
        rng = np.random.default_rng(9)
        seeds = _seed_list(rng, case.keys, 33, 3)
        hq.attach(case.ix, max_m=4)  # an IVF8_HNSW4-sized graph
        hq.set_quantizer_ef(case.ix, 1)
        _check(case, seeds, 10, 8, what="built graph, quantizer_ef = 1")
        # two rings of four cells with no edge between them: the walk from the entry point finds four of eight probes
        hq.attach(case.ix, max_m=2, graph=hqref.two_rings())
        _check(case, seeds, 10, 8, what="two rings")
        probes = case.ix.last_probes()
        assert probes.shape == (33, 8) and np.all(probes[:, 4:] == -1) and np.all(probes[:, :4] >= 0), "missing probes are exported as -1"
        assert hq.last_quantizer_stats(case.ix)["missing_probes"] == 4 * 33
    finally:
        case.close()


# ---- 6. a shard set ---------------------------------------------------------------------------------------------------------
class SetCase:
    prefix, has_ht, k_id = "shard_set", True, 5

    def __init__(self, pkg, fb, metric):
        self.pkg, self.fb = pkg, fb
        m = _metric(pkg, metric)
        d = 32
        self.x, self.keys = _data(41, d)
        x = self.x
        a = pkg.ivf_ann.FaissIvfFlat.train(m, NLIST, x[:800], niter=NITER)
        a.add(x[:800], self.keys[:800])
        b = pkg.ivfpq_ann.FaissIvfPq.train(m, NLIST, 8, x[600:1400], niter=NITER)
        b.add(x[600:1400], self.keys[600:1400])
        c = pkg.opq_ann.FaissOpqIvfPq.train(m, NLIST, 4, 16, x[1200:2000], niter=NITER)
        c.add(x[1200:2000], self.keys[1200:2000])
        dup = pkg.ivf_ann.FaissIvfFlat.load(m, a.centroids())  # the rows of the first member again, under other ids: ties
        dup.add(x[:800], np.arange(800, dtype=np.int64) - 400)
        self.members = [a, b, c, dup]
        self.ss = pkg.shard_set.ShardSet.create(m, d)
        self.ss.set_members(self.members)
        self.store = pkg.ann_by_id.EmbeddingStore.build(self.keys, self.x)

    def handle(self):
        return self.ss._h

    def plain(self, q, k, nprobe, ht=0):
        return self.ss.search(q, k, nprobe, ht)

    def close(self):
        self.ss.close()
        for mbr in self.members:
            mbr.close()
        self.store.close()


@pytest.mark.parametrize("metric", ["L2", "Cosine"])
def test_shard_set(pkg, fb, metric):
    case = SetCase(pkg, fb, metric)
    try:
        rng = np.random.default_rng(10)
        seeds = _seed_list(rng, case.keys[:800], 33, 4)  # rows the first and the last member both hold
        for k, nprobe in ((1, 1), (10, 8)):
            s, i, d, c = _check(case, seeds, k, nprobe, what=f"set {metric} k={k} nprobe={nprobe}")
            st = _stats(case)
            assert st["h2d_bytes"] == 8 * len(seeds) and st["found"] == 33 and st["absent"] == 4
            assert st["d2h_result_bytes"] == 20 * len(s) + 4 * len(seeds)
        ties = sum(1 for at in range(0, len(d) - 1) if s[at] == s[at + 1] and d[at] == d[at + 1] and i[at] != i[at + 1])
        assert ties >= 33, "the duplicate member ties with the first one, id by id"
        _check(case, _seed_list(rng, case.keys, 4130, 3), 2, 2)  # the set's own second chunk
        lib = fb._lib()
        rc, *_ = _raw(case, seeds, 10, 8, ht=20)
        assert rc == EINVAL and "IVF-Flat" in lib.ivf_by_id_last_error().decode()
        few = case.members[1:3]  # the members with codes: ht goes through
        case.ss.set_members(few)
        _check(case, seeds, 10, 8, ht=30)
    finally:
        case.close()


# ---- 7. determinism, the Python mirror -------------------------------------------------------------------------------------
def test_the_same_call_twice_returns_the_same_bytes(flat16, pq48):
    rng = np.random.default_rng(12)
    for case in (flat16, pq48):
        seeds = _seed_list(rng, case.keys, 200, 20)
        one = _raw(case, seeds, 10, 4)
        two = _raw(case, seeds, 10, 4)
        assert one[0] == 0 and one[5] == two[5]
        for a, b in zip(one[1:5], two[1:5]):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("kind,metric", [("flat", "Cosine"), ("sq8", "InnerProduct"), ("pq", "Cosine"), ("opq", "L2")])
def test_python_mirror_is_the_queryable_composition(pkg, fb, sq, hq, kind, metric):
    P = pkg.ivf_ann.FaissParams
    case = Case(pkg, fb, sq, kind, metric, 40 if kind == "opq" else 16, seed=51)
    try:
        m = _metric(pkg, metric)
        by_id = fb.FaissQueryableById(case.store, case.ix, m)
        seeds = _seed_list(np.random.default_rng(13), case.keys, 12, 3)
        params = P(nprobe=3, ht=40) if case.has_ht else P(nprobe=3)

        class Filtered:  # the index's search with ht, for FaissQueryable (which passes nprobe alone); the handle stays with case.ix
            def search(self, q, k, nprobe):
                return case.plain(q, k, nprobe, 40)

        plain = pkg.ivf_ann.FaissQueryable(Filtered() if case.has_ht else case.ix, m)
        want = []
        for sd in seeds.tolist():
            row, found = case.store.get([sd])
            if found[0]:
                want += [(sd, i, dist) for i, dist in plain.queryWithDistance(row[0], 10, P(nprobe=3))]
        got = by_id.batchQueryWithDistanceById(seeds, 10, params)
        assert got == want and len(got) > 0
        assert by_id.batchQueryById(seeds, 10, params) == [(s, i) for s, i, _ in want]
        assert by_id.queryByIdWithDistance(int(seeds[0]), 10, params) == [(i, d) for s, i, d in want if s == seeds[0]][:10]
        assert by_id.queryById(int(ABSENT[0]), 10, params) == []
        st = by_id.last_stats()
        assert st["found"] == 0 and st["absent"] == 1
        if kind in ("flat", "pq"):  # quantizerEf: refused without a graph, set through hnsw_quantizer with one
            with pytest.raises(ValueError, match="quantizerEf"):
                by_id.batchQueryById(seeds, 10, P(nprobe=3, quantizerEf=4))
            hq.attach(case.ix, max_m=4)
            walked = pkg.hnsw_quantizer.HnswQuantizedFaissQueryable(case.ix, m)
            p2 = P(nprobe=3, quantizerEf=4)
            want2 = []
            for sd in seeds.tolist():
                row, found = case.store.get([sd])
                if found[0]:
                    want2 += [(sd, i, dist) for i, dist in walked.queryWithDistance(row[0], 10, p2)]
            assert by_id.batchQueryWithDistanceById(seeds, 10, p2) == want2
            assert hq.info(case.ix)["quantizer_ef"] == 4
    finally:
        case.close()
