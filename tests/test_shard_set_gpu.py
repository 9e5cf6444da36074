"""include/shard_set.h on the device: a set of loaded indexes answers what the host composition of its members' own searches
answers, byte for byte.  Every comparison is an equality of bytes against dense_ann.compose (dann_compose_shards, whose
output buffers start as zeros), so no tolerance is chosen anywhere.

Shapes follow test_faiss_files_gpu.py: d = 32 (OPQ 48 -> 32), nlist = 8, M = 8, a few hundred rows per member, 5 queries.

One restriction on the data of the compose test, with its reason.  dann_compose_shards orders with std::sort and a
comparator under which (-0.0, id) and (+0.0, id) are equivalent; the order std::sort leaves equivalent elements in is
unspecified, so for two such entries of one query the reference itself is not defined byte for byte.  The sign of a zero
distance is therefore a function of the id: -0.0 and +0.0 still tie ACROSS ids (the tie must then go to the id, which an
ordering by the floats' bits would get wrong), and entries equal in distance and id are equal in every bit."""
import datetime as dt
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = ["flat", "pq", "opq"]
METRICS = ["L2", "Cosine", "InnerProduct"]
D, D_IN, NLIST, M, K, NPROBE = 32, 48, 8, 8, 10, 3
HT, K_HT = 26, 200  # of the 64 code bits; a few rows in a hundred pass (the tests assert that some do and some do not)
EINVAL = 1
UTC = dt.timezone.utc


def _metric(pkg, name):
    return getattr(pkg.dense_ann.DistanceMetric, name)


def _same(got, want, what=""):
    for name, g, w in zip(("ids", "distances", "counts"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert g.tobytes() == w.tobytes(), (what, name)


# ---- 1. the fold kernel on arbitrary runs -----------------------------------------------------------------------------------
POOL = np.array([-1.5, -0.0, 0.0, 0.25, 1.0, 3.5, np.inf], np.float32)
IDS = np.array([-(1 << 40), -7, -1, 0, 1, 2, 5, 1 << 31, (1 << 32) + 3, (1 << 32) + 4, 1 << 45, (1 << 62) + 1], np.int64)
COMPOSE_CASES = [(1, 1, 1), (2, 2, 2), (3, 31, 31), (17, 32, 32), (2, 33, 33), (3, 64, 64), (2, 512, 512), (3, 513, 513),
                 (2, 1023, 1023), (3, 1024, 1024), (17, 1024, 1024),
                 (3, 10, 64),     # k_in < k, and the total (<= 30) is below k
                 (3, 100, 10),    # k_in > k
                 (2, 1024, 1), (1, 5, 1024), (17, 64, 1000), (17, 3, 33), (2, 0, 5)]


def _runs(n_shards, k_in, nq, seed):
    rng = np.random.default_rng(seed)
    which = rng.integers(0, len(IDS), (n_shards, nq, k_in))
    ids = IDS[which]
    dist = POOL[rng.integers(0, len(POOL), (n_shards, nq, k_in))]
    zero = dist == 0
    dist[zero] = np.where(which[zero] % 2 == 0, np.float32(-0.0), np.float32(0.0))  # (the module docstring says why)
    cnt = rng.integers(0, k_in + 1, (n_shards, nq)).astype(np.int32)
    cnt[0, 0], cnt[-1, -1] = 0, k_in
    if n_shards > 1:
        cnt[:, 1] = 0  # a query nobody answers
        cnt[:, 2] = k_in  # and one everybody answers in full
    return [(ids[s], dist[s], cnt[s]) for s in range(n_shards)]


@pytest.mark.parametrize("n_shards,k_in,k", COMPOSE_CASES)
def test_compose_is_the_host_composition(pkg, n_shards, k_in, k):
    nq = 7
    runs = _runs(n_shards, k_in, nq, 1000 * n_shards + k_in + k)
    want = pkg.dense_ann.compose(runs, k)
    got = pkg.ShardSet.compose(runs, k)
    _same(got, want, (n_shards, k_in, k))
    total = np.stack([r[2] for r in runs]).sum(0)
    assert got[2].tolist() == np.minimum(total, k).tolist()
    if k_in >= 31 and k >= 31:  # the data does what it is there for: ties in distance and whole duplicates inside an answer
        q = int(np.argmax(got[2]))
        m = int(got[2][q])
        pairs = list(zip(got[1][q, :m].tolist(), got[0][q, :m].tolist()))
        assert len(set(pairs)) < len(pairs) and len({d for d, _ in pairs}) < len(set(pairs))


# ---- members ----------------------------------------------------------------------------------------------------------------
def _data(seed, d=D, n=2600, d_in=D_IN, M=M):
    """centroids [8, d]; rows around them; the same lifted to d_in dimensions through A^T (A [d, d_in], orthonormal rows), so
    that A x gives them back; 5 queries; PQ codebooks; ids."""
    rng = np.random.default_rng(seed)
    cent = (4.0 * np.eye(NLIST, d) + 0.3 * rng.standard_normal((NLIST, d))).astype(np.float32)
    cells = rng.integers(0, NLIST, n)
    rows = (cent[cells] + 0.1 * rng.standard_normal((n, d))).astype(np.float32)
    A = np.linalg.qr(rng.standard_normal((d_in, d)))[0].T.astype(np.float32)
    q = (cent[[1, 2, 3, 5, 7]] + 0.2 * rng.standard_normal((5, d))).astype(np.float32)
    return dict(cent=cent, rows=rows, rows_in=(rows @ A).astype(np.float32), A=A, q=q, q_in=(q @ A).astype(np.float32),
                cb=(0.1 * rng.standard_normal((M, 256, d // M))).astype(np.float32), ids=rng.permutation(10**6)[:n].astype(np.int64))


def _new(pkg, kind, metric, data):
    m = _metric(pkg, metric)
    if kind == "flat":
        return pkg.ivf_ann.FaissIvfFlat.load(m, data["cent"])
    if kind == "pq":
        return pkg.ivfpq_ann.FaissIvfPq.load(m, data["cent"], data["cb"])
    return pkg.opq_ann.FaissOpqIvfPq.load(m, data["A"], data["cent"], data["cb"])


def _dim(kind, data):
    return data["A"].shape[1] if kind == "opq" else data["cent"].shape[1]


def _loaded(pkg, kind, metric, data, a, b, path, ids=None):
    """Rows [a, b) in an index of the kind, written to the directory and loaded from it."""
    ix = _new(pkg, kind, metric, data)
    ix.add(data["rows_in" if kind == "opq" else "rows"][a:b], data["ids"][a:b] if ids is None else ids)
    pkg.faiss_files.write_index(ix, path)
    ix.close()
    return pkg.faiss_files.load_native_index(_dim(kind, data), _metric(pkg, metric), path)


def _q(kind, data):
    return data["q_in" if kind == "opq" else "q"]


def _member_search(pkg, member, q, k, nprobe, ht=0):
    return pkg.polysemous_ann.search_ht(member, q, k, nprobe, ht) if ht > 0 else member.search(q, k, nprobe)


def _composed(pkg, members, q, k, nprobe, ht=0):
    return pkg.dense_ann.compose([_member_search(pkg, m, q, k, nprobe, ht) for m in members], k)


def _close(*things):
    for t in things:
        t.close()


# ---- 2. each kind x each metric ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", KINDS)
def test_set_is_the_composition_of_its_members(pkg, tmp_path, kind, metric):
    data = _data(3)
    m300 = _loaded(pkg, kind, metric, data, 0, 300, tmp_path / "a")
    m500 = _loaded(pkg, kind, metric, data, 300, 800, tmp_path / "b")
    m1200 = _loaded(pkg, kind, metric, data, 800, 2000, tmp_path / "c")
    empty = _new(pkg, kind, metric, data)
    q = _q(kind, data)
    ss = pkg.ShardSet.create(_metric(pkg, metric), _dim(kind, data))
    members = [m1200, empty, m300, m500]
    ss.set_members(members)
    assert ss.info() == {"members": 4, "dimension": _dim(kind, data), "metric": _metric(pkg, metric), "rows": 2000}
    for k in (1, 10, 64):
        _same(ss.search(q, k, NPROBE), _composed(pkg, members, q, k, NPROBE), (kind, metric, k))
    # every list of every member: the members hold 1200, 0, 300 and 500 rows, so two counts fall below k = 1000 ...
    got = ss.search(q, 1000, 8)
    parts = [m.search(q, 1000, 8) for m in members]
    assert [p[2].tolist() for p in parts] == [[1000] * 5, [0] * 5, [300] * 5, [500] * 5]
    _same(got, pkg.dense_ann.compose(parts, 1000), (kind, metric, 1000))
    assert got[2].tolist() == [1000] * 5  # ... their union exceeds it,
    few = [m300, empty, m500]
    ss.set_members(few)
    got = ss.search(q, 1000, 8)
    _same(got, _composed(pkg, few, q, 1000, 8), (kind, metric, "800 rows"))
    assert got[2].tolist() == [800] * 5 and not got[0][:, 800:].any() and not got[1][:, 800:].any()  # and here falls short of it
    _close(ss, m300, m500, m1200, empty)


# ---- 3. ties across members ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["flat", "pq"])
def test_cross_member_ties(pkg, tmp_path, kind):
    data = _data(4)
    ids = np.arange(400, dtype=np.int64) * 3 + 1
    other = ids + np.where(np.arange(400) % 2 == 0, -1, 1)  # the same order, every id one lower or one higher
    a = _loaded(pkg, kind, "L2", data, 0, 400, tmp_path / "a", ids)
    b = pkg.faiss_files.load_native_index(D, _metric(pkg, "L2"), tmp_path / "a")
    c = _loaded(pkg, kind, "L2", data, 0, 400, tmp_path / "c", other)
    members = [a, b, c]
    ss = pkg.ShardSet.create(_metric(pkg, "L2"), D)
    ss.set_members(members)
    k = 30
    got = ss.search(data["q"], k, NPROBE)
    _same(got, _composed(pkg, members, data["q"], k, NPROBE), kind)
    equal_distance_other_id = whole_duplicates = 0
    for row_ids, row_dist, cnt in zip(*got):
        pairs = list(zip(row_dist[:cnt].tolist(), row_ids[:cnt].tolist()))
        whole_duplicates += len(pairs) - len(set(pairs))
        equal_distance_other_id += len(set(pairs)) - len({d for d, _ in pairs})
    assert equal_distance_other_id > 0 and whole_duplicates > 0
    _close(ss, a, b, c)


# ---- 4. mixed kinds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "Cosine"])
def test_mixed_kinds_in_one_set(pkg, tmp_path, metric):
    wide = _data(5, d=D_IN, n=900, M=12)  # flat and PQ members of dimension 48 (12 sub-quantizers of 4 components)
    lifted = _data(6, n=400)        # an OPQ member 48 -> 32
    flat = _loaded(pkg, "flat", metric, wide, 0, 300, tmp_path / "flat")
    pq = _loaded(pkg, "pq", metric, wide, 300, 900, tmp_path / "pq")
    opq = _loaded(pkg, "opq", metric, lifted, 0, 400, tmp_path / "opq")
    q = np.concatenate([wide["q"], lifted["q_in"]])
    members = [pq, opq, flat]
    ss = pkg.ShardSet.create(_metric(pkg, metric), D_IN)
    ss.set_members(members)
    for k in (10, 200):
        _same(ss.search(q, k, NPROBE), _composed(pkg, members, q, k, NPROBE), (metric, k))
    _close(ss, flat, pq, opq)


# ---- 5. ht ------------------------------------------------------------------------------------------------------------------
def test_ht_goes_to_the_members_that_have_codes(pkg, tmp_path):
    data = _data(7, d_in=D)  # OPQ 32 -> 32: every member has dimension 32 and 8 sub-quantizers
    pq = _loaded(pkg, "pq", "L2", data, 0, 600, tmp_path / "pq")
    opq = _loaded(pkg, "opq", "L2", data, 600, 1300, tmp_path / "opq")
    opq2 = _loaded(pkg, "opq", "L2", data, 1300, 1600, tmp_path / "opq2")
    flat = _loaded(pkg, "flat", "L2", data, 1600, 1900, tmp_path / "flat")
    q = np.concatenate([data["q"], data["q_in"]])
    members = [pq, opq, opq2]
    ss = pkg.ShardSet.create(_metric(pkg, "L2"), D)
    ss.set_members(members)
    k = K_HT
    plain = ss.search(q, k, NPROBE)
    _same(plain, _composed(pkg, members, q, k, NPROBE), "ht = 0")
    got = ss.search(q, k, NPROBE, HT)
    _same(got, _composed(pkg, members, q, k, NPROBE, HT), f"ht = {HT}")
    print(f"ht = {HT}: counts {got[2].tolist()} against {plain[2].tolist()} unfiltered")
    assert 0 < got[2].sum() < plain[2].sum(), "the filter must drop some rows and keep some"
    _same(ss.search(q, k, NPROBE, -3), plain, "ht < 0 is no filter")
    # an IVF-Flat member has no codes to filter by: refused before any work, and the set goes on answering
    ss.set_members(members + [flat])
    with pytest.raises(pkg.shard_set.ShardSetError, match="IVF-Flat") as e:
        ss.search(q, k, NPROBE, HT)
    assert e.value.code == EINVAL
    _same(ss.search(q, k, NPROBE), _composed(pkg, members + [flat], q, k, NPROBE), "after the refusal")
    _close(ss, pq, opq, opq2, flat)


# ---- 6. membership ------------------------------------------------------------------------------------------------------------
def test_membership(pkg, tmp_path):
    data = _data(9)
    a = _loaded(pkg, "flat", "L2", data, 0, 300, tmp_path / "a")
    b = _loaded(pkg, "pq", "L2", data, 300, 700, tmp_path / "b")
    c = _loaded(pkg, "flat", "L2", data, 700, 1000, tmp_path / "c")
    cosine = _loaded(pkg, "flat", "Cosine", data, 0, 300, tmp_path / "cosine")
    wide = _data(10, d=D_IN, n=300, M=12)
    other_d = _loaded(pkg, "flat", "L2", wide, 0, 300, tmp_path / "wide")
    q = data["q"]
    own_before = a.search(q, K, NPROBE)
    ss = pkg.ShardSet.create(_metric(pkg, "L2"), D)
    _same(ss.search(q, K, NPROBE), (np.zeros((5, K), np.int64), np.zeros((5, K), np.float32), np.zeros(5, np.int32)), "a new set")
    ss.set_members([a, b])
    first = ss.search(q, K, NPROBE)
    _same(first, _composed(pkg, [a, b], q, K, NPROBE), "a, b")
    for bad, word in [(cosine, "metric"), (other_d, "dimension")]:
        with pytest.raises(pkg.shard_set.ShardSetError, match=word) as e:
            ss.set_members([a, bad, b])
        assert e.value.code == EINVAL
        assert ss.info()["members"] == 2 and ss.members == [a, b]
        _same(ss.search(q, K, NPROBE), first, f"after the refused {word}")
    closed = _new(pkg, "flat", "L2", data)
    closed.close()
    with pytest.raises(pkg.shard_set.ShardSetError, match="null handle"):
        ss.set_members([closed])
    ss.set_members([c, b])
    second = ss.search(q, K, NPROBE)
    _same(second, _composed(pkg, [c, b], q, K, NPROBE), "c, b")
    assert second[0].tobytes() != first[0].tobytes()
    _same(a.search(q, K, NPROBE), own_before, "a member's own search after the set used it")
    ss.set_members([])
    none = ss.search(q, K, NPROBE)
    assert none[2].tolist() == [0] * 5 and not none[0].any() and not none[1].any() and ss.info()["rows"] == 0
    with pytest.raises(pkg.shard_set.ShardSetError, match="k must"):
        ss.search(q, 1025, NPROBE)
    _close(ss, a, b, c, cosine, other_d)


# ---- 7. chunks and the bytes that cross the bus ---------------------------------------------------------------------------------
def test_chunking_and_stats(pkg, tmp_path):
    data = _data(11)
    a = _loaded(pkg, "flat", "L2", data, 0, 300, tmp_path / "a")
    b = _loaded(pkg, "pq", "L2", data, 300, 700, tmp_path / "b")
    c = _loaded(pkg, "flat", "L2", data, 700, 1000, tmp_path / "c")
    rng = np.random.default_rng(12)
    nq = 4097  # one more than a chunk
    q = (data["cent"][rng.integers(0, NLIST, nq)] + 0.2 * rng.standard_normal((nq, D))).astype(np.float32)
    ss = pkg.ShardSet.create(_metric(pkg, "L2"), D)
    control = []
    for members in ([a], [a, b, c]):
        ss.set_members(members)
        got = ss.search(q, K, NPROBE)
        _same(got, _composed(pkg, members, q, K, NPROBE), len(members))
        st = ss.last_stats()
        assert st["h2d_bytes"] == 4 * nq * D and st["d2h_result_bytes"] == 12 * nq * K + 4 * nq, st
        assert st["d2h_bytes"] > st["d2h_result_bytes"] and st["search_ms"] > 0 and st["fold_ms"] > 0, st
        control.append(st["d2h_bytes"] - st["d2h_result_bytes"])
        _same(ss.search(q, K, NPROBE), got, "the same call again")
    assert control[0] < control[1] < 4096  # control words only, more of them with more members
    _close(ss, a, b, c)


# ---- 8. the hourly holder -------------------------------------------------------------------------------------------------------
def test_hourly_sharded_index_searches_through_the_set(pkg, tmp_path):
    ff, ps = pkg.faiss_files, pkg.polysemous_ann
    m = _metric(pkg, "L2")
    rng = np.random.default_rng(13)
    rows = rng.standard_normal((1200, D)).astype(np.float32)
    ids = np.arange(1200, dtype=np.int64) * 3 + 1
    q = rows[[10, 350, 620, 100, 500]] + 0.05 * rng.standard_normal((5, D)).astype(np.float32)
    now = dt.datetime(2024, 1, 1, 1, 30, tzinfo=UTC)
    root = tmp_path / "root"
    for back, (lo, hi) in enumerate([(0, 300), (300, 700), (700, 1200)]):
        directory = str(root / (now - dt.timedelta(hours=back)).strftime("%Y/%m/%d/%H"))
        os.makedirs(os.path.dirname(directory), exist_ok=True)
        ff.build_and_write_faiss_index(rows[lo:hi], ids[lo:hi], 1.0, "IVF8,PQ8", m, directory, niter=2, seed=5)
    sh = ff.HourlyShardedIndex(m, D, root, 3, 24)
    assert sh.reload(now) is True and sh.loads == 3
    k = K_HT
    plain = sh.search(q, k, NPROBE)
    _same(plain, sh.search_composed(q, k, NPROBE), "ht = 0")
    got = sh.search(q, k, NPROBE, HT)
    _same(got, sh.search_composed(q, k, NPROBE, HT), f"ht = {HT}")
    print(f"ht = {HT}: counts {got[2].tolist()} against {plain[2].tolist()} unfiltered")
    assert 0 < got[2].sum() < plain[2].sum(), "the filter must drop some rows and keep some"
    pairs = ps.PolysemousFaissQueryable(sh, m).queryWithDistance(q[0], k, pkg.ivf_ann.FaissParams(nprobe=NPROBE, ht=HT))
    one = sh.search(q[:1], k, NPROBE, HT)
    assert [i for i, _ in pairs] == one[0][0, :one[2][0]].tolist() and [d for _, d in pairs] == one[1][0, :one[2][0]].tolist()
    sh.close()
    assert sh.closes == 3
