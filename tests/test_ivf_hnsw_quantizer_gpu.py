"""The HNSW coarse quantizer of the IVF family on the device (include/ivf_hnsw_quantizer.h).

What is held: the probes of a search ARE the graph's walk (id for id against hnsw_search over the borrowed graph and against
the CPU oracle's walk over the exported graph), the cells of an add are the k = 1 walk, the answers keep the contract of the
index they come from (the float64 restatements of tests/_ivf_ref.py and tests/_ivfpq_ref.py, fed with the exported
centroids, assignment and probes, with their tolerances as they are), a short walk is no error, and everything layered on
the core (ShardSet, the device-output search, the directory) sees the same index.  L2 and InnerProduct rows and queries
are fp16-representable, so that every preparation is the identity; Cosine goes through last_queries and the stored rows."""
import importlib

import numpy as np
import pytest

import _ivf_ref as ref
import _ivfhq_ref as hqref
import _ivfpq_ref as pqref
import _polysemous_ref as polyref

pytestmark = pytest.mark.gpu

N, NQ = 3000, 70
METRICS = ["L2", "Cosine", "InnerProduct"]


@pytest.fixture(scope="module")
def hq(pkg):
    return importlib.import_module(pkg.__name__ + ".hnsw_quantizer")


def _metric(pkg, name):
    return getattr(pkg.dense_ann.DistanceMetric, name)


def _data(d, nlist, seed, n=N, nq=NQ):
    rng = np.random.default_rng(seed)
    x = hqref.fp16_rows(rng, n + nq, d)
    M = 4 if d == 16 else 8
    return dict(x=x[:n], q=x[n:], ids=rng.permutation(n).astype(np.int64) * 3 + 7, cent=x[rng.choice(n, nlist, replace=False)],
                cb=(rng.integers(-64, 65, (M, 256, d // M)) / 64.0).astype(np.float32), M=M)


def _new(pkg, kind, metric, data):
    m = _metric(pkg, metric)
    if kind == "flat":
        return pkg.ivf_ann.FaissIvfFlat.load(m, data["cent"])
    if kind == "pq":
        return pkg.ivfpq_ann.FaissIvfPq.load(m, data["cent"], data["cb"])
    d = data["cent"].shape[1]
    return pkg.opq_ann.FaissOpqIvfPq.load(m, np.eye(d, dtype=np.float32), data["cent"], data["cb"])


def _built(pkg, hq, kind, metric, data, max_m, rows=True):
    ix = _new(pkg, kind, metric, data)
    hq.attach(ix, max_m=max_m)
    assert hq.info(ix) == {"attached": True, "max_m": max_m, "quantizer_ef": 16}
    if rows:
        ix.add(data["x"], data["ids"])
    return ix


def _same(a, b, what=""):
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), what


def _walks(nlist):
    """(nprobe, quantizer_ef): nprobe 1, 8, nlist and 1024 (clamped); ef 1, 16, 64; nprobe above ef (the beam is the larger)."""
    return [(1, 1), (8, 16), (nlist, 1), (1024, 64), (8, 1), (1, 64)]


def _check_probes_are_the_walk(pkg, hq, oracle, ix, metric, q, identity):
    view = hq.quantizer(ix)
    graph, cent = view.graph(), ix.centroids()
    assert np.array_equal(view.stored_vectors(), cent), "the graph's vectors are the stored centroids"
    assert int(view.metric) == hqref.graph_metric(_metric(pkg, metric)) and view.n == ix.nlist
    for nprobe, ef in _walks(ix.nlist):
        hq.set_quantizer_ef(ix, ef)
        ix.search(q, 5, nprobe)
        probes, lq = ix.last_probes(), hq.last_queries(ix)
        kk = min(nprobe, ix.nlist)
        assert probes.shape == (len(q), kk) and lq.shape == (len(q), ix.d)
        if identity:
            assert np.array_equal(lq, q), "an L2 / InnerProduct preparation of fp16 values is the identity"
        else:
            assert np.array_equal(lq, lq.astype(np.float16).astype(np.float32))
        st = hq.last_quantizer_stats(ix)
        ids, _, cnt = view.search(lq, kk, ef)
        assert np.array_equal(probes, hqref.padded(ids, cnt)), (nprobe, ef, "hnsw_search over the borrowed graph")
        o_cells, o_cnt = hqref.oracle_walk(oracle, _metric(pkg, metric), cent, graph, lq, kk, ef)
        assert np.array_equal(probes, o_cells), (nprobe, ef, "the CPU oracle's walk")
        assert st["missing_probes"] == int((probes < 0).sum()) and st["distance_evals"] > 0
        assert ix.last_stats()["rows_scanned"] == hqref.rows_probed(ix)


# ---- 1. probes are the walk ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind,d,nlist,max_m", [("flat", 16, 64, 8), ("flat", 64, 300, 2), ("flat", 16, 1, 2),
                                                 ("pq", 64, 300, 8), ("pq", 16, 64, 2)])
def test_probes_are_the_walk(pkg, hq, oracle, kind, d, nlist, max_m, metric):
    data = _data(d, nlist, 10 + d + nlist)
    ix = _built(pkg, hq, kind, metric, data, max_m)
    _check_probes_are_the_walk(pkg, hq, oracle, ix, metric, data["q"], metric != "Cosine")
    ix.close()


def test_probes_are_the_walk_opq(pkg, hq, oracle):
    data = _data(64, 64, 21)
    ix = _built(pkg, hq, "opq", "L2", data, 8)
    _check_probes_are_the_walk(pkg, hq, oracle, ix, "L2", data["q"], True)
    ix.close()


def test_probes_across_a_chunk_boundary(pkg, hq, oracle):
    """4,097 queries: the second chunk of the search holds one query."""
    data = _data(16, 64, 22, nq=4097)
    ix = _built(pkg, hq, "flat", "L2", data, 8)
    view = hq.quantizer(ix)
    got = ix.search(data["q"], 3, 8)
    probes = ix.last_probes()
    assert probes.shape == (4097, 8) and np.array_equal(hq.last_queries(ix), data["q"])
    ids, _, cnt = view.search(data["q"], 8, 16)
    assert np.array_equal(probes, hqref.padded(ids, cnt))
    tail = slice(4000, 4097)
    o_cells, _ = hqref.oracle_walk(oracle, 0, ix.centroids(), view.graph(), data["q"][tail], 8, 16)
    assert np.array_equal(probes[tail], o_cells)
    # the query of the second chunk answers as it does alone
    _same([a[4096:] for a in got], ix.search(data["q"][4096:], 3, 8))
    ix.close()


# ---- 2. assignment is the walk ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,metric", [("flat", "L2"), ("flat", "InnerProduct"), ("flat", "Cosine"), ("pq", "L2"),
                                         ("pq", "InnerProduct")])
def test_assignment_is_the_walk(pkg, hq, oracle, kind, metric):
    data = _data(16, 64, 30)
    ix = _built(pkg, hq, kind, metric, data, 2, rows=False)
    view = hq.quantizer(ix)
    hq.set_quantizer_ef(ix, 64)
    ix.add(data["x"][:2000], data["ids"][:2000])
    hq.set_quantizer_ef(ix, 1)
    ix.add(data["x"][2000:], data["ids"][2000:])  # the second add walks at the new ef
    got_ids, cells = ix.assignment()
    assert np.array_equal(got_ids, data["ids"])
    rows = pkg.faiss_files.stored_rows(ix).astype(np.float32) if metric == "Cosine" else data["x"]
    want = np.concatenate([view.search(rows[:2000], 1, 64)[0][:, 0], view.search(rows[2000:], 1, 1)[0][:, 0]])
    assert np.array_equal(cells, want)
    assert not np.array_equal(view.search(rows[2000:], 1, 64)[0][:, 0], want[2000:]), "ef = 1 and ef = 64 assign differently here"
    o_cells, _ = hqref.oracle_walk(oracle, _metric(pkg, metric), ix.centroids(), view.graph(), rows[1900:2100], 1, 64)
    assert np.array_equal(cells[1900:2000], o_cells[:100, 0])
    o_cells, _ = hqref.oracle_walk(oracle, _metric(pkg, metric), ix.centroids(), view.graph(), rows[2000:2100], 1, 1)
    assert np.array_equal(cells[2000:2100], o_cells[:, 0])
    assert np.array_equal(ix.list_sizes(), np.bincount(cells, minlength=64))
    ix.close()


# ---- 3. answers keep their contract -------------------------------------------------------------------------------------
def _spread(d, nlist, seed):
    """Rows whose distances spread (tests/_ivf_ref.low_dimensional), so that few positions of a comparison are unclear."""
    rng = np.random.default_rng(seed)
    x = ref.low_dimensional(rng, N + 33, d)
    M = 4 if d == 16 else 8
    return dict(x=x[:N], q=x[N:], ids=rng.permutation(N).astype(np.int64) * 5 + 2, cent=x[rng.choice(N, nlist, replace=False)],
                cb=(0.1 * rng.standard_normal((M, 256, d // M))).astype(np.float32), M=M)


def _train_pq(pkg, metric, data):
    """Centroids and codebooks trained on the rows, as tests/test_ivfpq_gpu.py trains them: random codewords would leave
    the scores of a list crowded within the tolerance."""
    trained = pkg.ivfpq_ann.FaissIvfPq.train(_metric(pkg, metric), len(data["cent"]), data["M"], data["x"][:1000], niter=2, seed=3)
    data["cent"], data["cb"] = trained.centroids(), trained.codebooks()
    trained.close()
    return data


@pytest.mark.parametrize("metric", METRICS)
def test_flat_answers_keep_their_contract(pkg, hq, metric):
    m = _metric(pkg, metric)
    data = _spread(64, 64, 40)
    ix = _built(pkg, hq, "flat", metric, data, 8)
    ids, cells = ix.assignment()
    for nprobe, ef, k in [(1, 16, 10), (8, 16, 10), (8, 1, 100), (64, 64, 200)]:
        hq.set_quantizer_ef(ix, ef)
        got = ix.search(data["q"], k, nprobe)
        unclear, total = hqref.check_flat(m, ref.prepare(int(m), data["x"]), ids, cells, ix.last_probes(), ref.prepare(int(m), data["q"]), k, got)
        print(f"{metric} nprobe={nprobe} ef={ef} k={k}: unclear positions {unclear} of {total}")
        assert unclear <= hqref.MAX_UNCLEAR * total, "the comparison would be vacuous"
        assert ix.last_stats()["rows_scanned"] == hqref.rows_probed(ix)
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_pq_answers_keep_their_contract(pkg, hq, metric):
    m = _metric(pkg, metric)
    data = _train_pq(pkg, metric, _spread(64, 64, 41))
    ix = _built(pkg, hq, "pq", metric, data, 8)
    ids, cells = ix.assignment()
    M, dsub = ix.M, ix.d // ix.M
    pq_ = ref.prepare(int(m), data["q"])
    for nprobe, ef, k in [(1, 16, 10), (8, 1, 10), (64, 64, 100)]:
        hq.set_quantizer_ef(ix, ef)
        got = ix.search(data["q"], k, nprobe)
        unclear, total = hqref.check_pq(m, M, dsub, ix.centroids(), ix.codebooks(), ix.codes(), ids, cells, ix.last_probes(), pq_, k, got)
        print(f"{metric} nprobe={nprobe} ef={ef} k={k}: unclear positions {unclear} of {total}")
        assert unclear <= hqref.MAX_UNCLEAR * total, "the comparison would be vacuous"
        assert ix.last_stats()["rows_scanned"] == hqref.rows_probed(ix)
    # ivfpq_search_ht at one ht: the filter applied in numpy to the unfiltered answer that lists every probed row
    hq.set_quantizer_ef(ix, 16)
    nprobe, k, ht = 8, 10, 4 * M
    all_ids, all_dist, all_cnt = ix.search(data["q"], 1024, nprobe)
    probes = ix.last_probes()
    probed = np.array([ix.list_sizes()[p].sum() for p in hqref.found(probes)])
    assert probed.max() <= 1024 and np.array_equal(all_cnt, probed)
    got = pkg.polysemous_ann.search_ht(ix, data["q"], k, nprobe, ht)
    assert np.array_equal(ix.last_probes(), probes)
    row_of = {int(i): r for r, i in enumerate(ids.tolist())}
    qcodes = np.empty((len(data["q"]), probes.shape[1], M), np.uint8)
    lib = pkg.polysemous_ann._lib()
    assert lib.ivfpq_last_query_codes(ix._h, None, None, qcodes.ctypes.data) == 0
    w_ids, w_dist, w_cnt, passed = polyref.filter_answer(all_ids, all_dist, all_cnt, row_of, ix.codes(), cells, probes, qcodes, ht, k)
    _same(got, (w_ids, w_dist, w_cnt), "ht")
    ix.close()


def test_opq_answers_keep_their_contract(pkg, hq):
    m = _metric(pkg, "L2")
    data = _train_pq(pkg, "L2", _spread(64, 64, 42))
    ix = _built(pkg, hq, "opq", "L2", data, 8)
    ids, cells = ix.assignment()
    for nprobe, ef, k in [(8, 16, 10), (64, 1, 100)]:
        hq.set_quantizer_ef(ix, ef)
        got = ix.search(data["q"], k, nprobe)
        prepared = pqref.prepare(int(m), ix.transform(data["q"]))
        assert np.array_equal(hq.last_queries(ix), prepared)
        unclear, total = hqref.check_pq(m, ix.M, ix.d // ix.M, ix.centroids(), ix.codebooks(), ix.codes(), ids, cells,
                                        ix.last_probes(), prepared, k, got)
        assert unclear <= hqref.MAX_UNCLEAR * total, "the comparison would be vacuous"
        assert ix.last_stats()["rows_scanned"] == hqref.rows_probed(ix)
    ix.close()


# ---- 4. a short walk ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["flat", "pq"])
def test_a_short_walk_is_not_an_error(pkg, hq, kind):
    m = _metric(pkg, "L2")
    rng = np.random.default_rng(50)
    d, nq, k = 16, 33, 200
    cent = np.zeros((8, d), np.float32)
    for c in range(8):
        cent[c, c] = 4.0
    cells = np.repeat(np.arange(8), [40, 30, 0, 50, 60, 300, 10, 20])
    x = (cent[cells] + rng.integers(-32, 33, (len(cells), d)) / 64.0).astype(np.float32)
    ids = rng.permutation(len(x)).astype(np.int64) * 2 + 1
    q = (cent[rng.integers(0, 8, nq)] + rng.integers(-32, 33, (nq, d)) / 64.0).astype(np.float32)
    data = dict(cent=cent, cb=(rng.integers(-32, 33, (4, 256, 4)) / 64.0).astype(np.float32))
    ix = _new(pkg, kind, "L2", data)
    ix.add(x, ids)  # assigned by the exhaustive search: an attach governs later adds and searches only
    assert np.array_equal(ix.assignment()[1], cells)
    hq.attach(ix, max_m=2, graph=hqref.two_rings())
    got = ix.search(q, k, 8)
    probes = ix.last_probes()
    assert probes.shape == (nq, 8) and np.all(probes[:, 4:] == -1)
    assert np.all(np.sort(probes[:, :4], axis=1) == np.arange(4)), "the four cells of the entry point's ring, each once"
    assert hq.last_quantizer_stats(ix)["missing_probes"] == 4 * nq
    assert ix.last_stats()["rows_scanned"] == 120 * nq
    assert np.all(got[2] == 120), "the four lists hold 120 rows: the counts fall short of k"
    if kind == "flat":
        hqref.check_flat(m, x, ids, cells, probes, q, k, got)
        exact = ref.search_probed(0, x, ids, cells, [np.arange(4)] * nq, q, k)
        for qi, (r_ids, _, _) in enumerate(exact):
            assert set(got[0][qi, :120].tolist()) == set(r_ids.tolist())
    else:
        hqref.check_pq(m, 4, 4, ix.centroids(), ix.codebooks(), ix.codes(), ids, cells, probes, q, k, got)
        _same(pkg.polysemous_ann.search_ht(ix, q, k, 8, 8 * 4 + 1), got, "the filtered scan ignores the missing probes too")
    with pytest.raises(hq.HnswQuantizerError):
        lv, it, off, nb, e, ml = hqref.two_rings()
        hq.attach(ix, max_m=2, graph=(lv, it, off, np.where(nb == 7, 8, nb), e, ml))
    assert hq.info(ix)["attached"] and np.array_equal(ix.search(q, k, 8)[0], got[0]), "a refusal changes nothing"
    ix.close()


# ---- 5. determinism and reversibility -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["flat", "pq"])
def test_determinism_and_reversibility(pkg, hq, kind):
    data = _data(64, 300, 60)
    a = _built(pkg, hq, kind, "L2", data, 8)
    b = _built(pkg, hq, kind, "L2", data, 8)
    twin = _new(pkg, kind, "L2", data)
    for u, v in zip(hq.quantizer(a).graph(), hq.quantizer(b).graph()):
        assert np.array_equal(u, v), "two builds of one input give one graph"
    _same(a.search(data["q"], 10, 8), b.search(data["q"], 10, 8))
    assert np.array_equal(a.last_probes(), b.last_probes()) and np.array_equal(a.assignment()[1], b.assignment()[1])
    # a batch of queries equals the same queries asked one at a time
    batch = a.search(data["q"][:9], 10, 8)
    probes = a.last_probes()
    for i in range(9):
        _same([r[i:i + 1] for r in batch], a.search(data["q"][i:i + 1], 10, 8), i)
        assert np.array_equal(a.last_probes(), probes[i:i + 1])
    # attach, then detach: the exhaustive index again, byte for byte
    with pytest.raises(hq.HnswQuantizerError):
        hq.set_quantizer_ef(twin, 16)
    hq.attach(twin, max_m=8)
    hq.detach(twin)
    assert hq.info(twin) == {"attached": False, "max_m": 0, "quantizer_ef": 16} and hq.quantizer(twin) is None
    never = _new(pkg, kind, "L2", data)
    twin.add(data["x"], data["ids"])
    never.add(data["x"], data["ids"])
    assert np.array_equal(twin.assignment()[1], never.assignment()[1])
    _same(twin.search(data["q"], 10, 8), never.search(data["q"], 10, 8))
    assert np.array_equal(twin.last_probes(), never.last_probes()) and hq.last_queries(twin).shape[0] == 0
    for ix in (a, b, twin, never):
        ix.close()


# ---- 6. layers above ----------------------------------------------------------------------------------------------------
def test_shard_set_of_quantized_members(pkg, hq):
    data = _data(64, 64, 70)
    flat = _built(pkg, hq, "flat", "L2", data, 8)
    pq = _built(pkg, hq, "pq", "L2", data, 2)
    hq.set_quantizer_ef(pq, 1)
    q = data["q"]
    ss = pkg.ShardSet.create(_metric(pkg, "L2"), 64)
    for members in ([flat], [pq], [flat, pq]):
        ss.set_members(members)
        for k, nprobe in ((10, 8), (200, 64)):
            # (a set of one member: the member's device-output search against its host-output search)
            want = pkg.dense_ann.compose([m.search(q, k, nprobe) for m in members], k)
            _same(ss.search(q, k, nprobe), want, (len(members), k, nprobe))
    ss.close()
    flat.close()
    pq.close()


# ---- 7. disk ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["flat", "pq", "opq"])
def test_save_and_load(pkg, hq, tmp_path, kind):
    data = _data(64, 64, 80)
    m = _metric(pkg, "L2")
    ix = _built(pkg, hq, kind, "L2", data, 8)
    hq.set_quantizer_ef(ix, 3)
    hq.write_index(ix, tmp_path / "a")
    assert pkg.faiss_files.is_valid_faiss_index(tmp_path / "a") and (tmp_path / "a" / hq.QUANTIZER_FILE_NAME).exists()
    back = hq.load_index(64, m, tmp_path / "a")
    assert type(back) is type(ix) and hq.info(back) == {"attached": True, "max_m": 8, "quantizer_ef": 16}
    for u, v in zip(hq.quantizer(back).graph(), hq.quantizer(ix).graph()):
        assert np.array_equal(u, v), "the graph entry for entry"
    hq.set_quantizer_ef(back, 3)
    _same(back.search(data["q"], 10, 8), ix.search(data["q"], 10, 8))
    assert np.array_equal(back.last_probes(), ix.last_probes())
    # the old loader: a valid exhaustive index, the detached twin
    old = pkg.faiss_files.FaissIndex.load_index(64, m, tmp_path / "a").index
    assert not hq.info(old)["attached"]
    hq.detach(ix)
    _same(old.search(data["q"], 10, 8), ix.search(data["q"], 10, 8))
    assert np.array_equal(old.last_probes(), ix.last_probes())
    for i in (ix, back, old):
        i.close()


# ---- 8. the factory strings, built and served ---------------------------------------------------------------------------
@pytest.mark.parametrize("string,cls", [("IVF16_HNSW4,Flat", "FaissIvfFlat"), ("IVF16_HNSW4,PQ8", "FaissIvfPq"),
                                        ("OPQ8,IVF16_HNSW4,PQ8", "FaissOpqIvfPq"), ("IVF16_HNSW4,PQ8,RFlat", "FaissRefineFlat")])
def test_build_faiss_index_and_the_queryable(pkg, hq, string, cls):
    m = _metric(pkg, "Cosine")
    rng = np.random.default_rng(90)
    x = ref.low_dimensional(rng, 1233, 32)
    ids = rng.permutation(1200).astype(np.int64) + 100
    ix = hq.build_faiss_index(x[:1200], ids, 0.5, string, m, niter=2)
    assert type(ix).__name__ == cls and ix.n == 1200
    assert hq.info(ix) == {"attached": True, "max_m": 4, "quantizer_ef": 16}
    holder = ix.base if cls == "FaissRefineFlat" else ix
    # the rows went through the quantizer: every cell is the k = 1 walk of the row the index prepared
    view = hq.quantizer(ix)
    assert view.n == 16 and view.max_m == 4
    qa = hq.HnswQuantizedFaissQueryable(ix, m)
    params = pkg.ivf_ann.FaissParams(nprobe=4, quantizerEf=7)
    for q in x[1200:1205]:
        got = qa.queryWithDistance(q, 5, params)
        assert hq.info(ix)["quantizer_ef"] == 7
        r_ids, r_dist, r_cnt = ix.search(q, 5, 4)
        assert [i for i, _ in got] == r_ids[0, :r_cnt[0]].tolist()
        lq = hq.last_queries(ix)
        w_ids, _, w_cnt = view.search(lq, 4, 7)
        assert np.array_equal(holder.last_probes(), hqref.padded(w_ids, w_cnt))
    qa.queryWithDistance(x[1200], 5, pkg.ivf_ann.FaissParams(nprobe=4))
    assert hq.info(ix)["quantizer_ef"] == 7, "None leaves it as it is"
    with pytest.raises(ValueError, match="quantizerNprobe"):
        qa.queryWithDistance(x[1200], 5, pkg.ivf_ann.FaissParams(nprobe=4, quantizerNprobe=2))
    ix.close()
