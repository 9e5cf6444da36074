"""Polysemous codes and the Hamming-filtered search on the device (include/polysemous_ann.h) against the restatement
tests/_polysemous_ref.py, fed with what the index exports: the unfiltered search's own answer over every row of the probed
lists, the codes, the assignment, the probes and the query codes.  A row that passes the filter must carry the bits the
unfiltered search gives it, so every comparison of answers here is byte for byte.

Shapes: d = 32, M = 8, nlist = 8, n = 2000 and nprobe = 2 unless a test says otherwise -- lists of about 250 rows (several
64-row blocks and a partial one) and at most 1024 rows in a query's probed lists, so that ivfpq_search with k = 1024 lists
them all; the tests assert that condition.  Speed and recall of the filter are not measured here."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import _ivfpq_ref as pq
import _polysemous_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ["L2", "Cosine", "InnerProduct"]
REF_METRIC = {"L2": pq.L2, "Cosine": pq.COSINE, "InnerProduct": pq.INNER_PRODUCT}
EINVAL = 1
ANNEAL = 2000  # annealing steps per subspace: the filter is exact whatever the numbering, training quality is not the point
# name -> (d, M, nlist, n, nprobe)
SHAPES = {"m8": (32, 8, 8, 2000, 2), "m4": (16, 4, 8, 2000, 2), "m48": (96, 48, 8, 2000, 2), "m64": (512, 64, 2, 600, 2)}


def _metric(pkg, name):
    return getattr(pkg.dense_ann.DistanceMetric, name)


def _data(shape, metric, nq=33):
    d, M, nlist, n, nprobe = SHAPES[shape]
    rng = np.random.default_rng(900 + 7 * list(SHAPES).index(shape) + METRICS.index(metric))
    centres = rng.standard_normal((nlist, d)) * 0.7
    x = (centres[rng.integers(0, nlist, n + nq)] + rng.standard_normal((n + nq, d))).astype(np.float32)
    ids = rng.permutation(n).astype(np.int64) * 5 + 2
    return x[:n], x[n:], ids


_CACHE = {}


@pytest.fixture(scope="module")
def built(pkg):
    """(index trained polysemous and filled, x, queries, ids) of a shape and metric, shared by the tests."""
    def get(shape, metric):
        key = (shape, metric)
        if key not in _CACHE:
            d, M, nlist, n, nprobe = SHAPES[shape]
            x, q, ids = _data(shape, metric)
            ix = pkg.polysemous_ann.PolysemousIvfPq.train(_metric(pkg, metric), nlist, M, x, niter=3, seed=5, anneal_iters=ANNEAL)
            ix.add(x, ids)
            _CACHE[key] = (ix, x, q, ids)
        return _CACHE[key]

    yield get
    for entry in _CACHE.values():
        entry[0].close()
    _CACHE.clear()


def _same(got, want, what):
    for u, v, name in zip(got, want, ("ids", "distances", "counts")):
        assert u.dtype == v.dtype and u.tobytes() == v.tobytes(), f"{what}: {name} differ"


def _check_filter(pkg, ix, q, ids, k, nprobe, hts):
    """Case 1 of the issue over either index type: every ht of hts against the filter applied in numpy to the unfiltered
    answer with k = 1024; 8M + 1, 0 and -3 against the unfiltered answer with k outright."""
    base = pkg.opq_ann.FaissOpqIvfPq if isinstance(ix, pkg.opq_ann.FaissOpqIvfPq) else pkg.ivfpq_ann.FaissIvfPq
    M = ix.M
    all_ids, all_dist, all_cnt = base.search(ix, q, 1024, nprobe)
    probes, plain_stats = ix.last_probes(), ix.last_stats()
    probed_rows = ix.list_sizes()[probes].sum(axis=1)
    assert probed_rows.max() <= 1024 and np.array_equal(all_cnt, probed_rows), "k = 1024 lists every row of the probed lists"
    assert plain_stats["rows_scanned"] == int(probed_rows.sum()) and plain_stats["rounds"] == 1
    plain = base.search(ix, q, k, nprobe)
    codes, (row_ids, cells) = ix.codes(), ix.assignment()
    assert np.array_equal(row_ids, ids)
    row_of = {int(i): r for r, i in enumerate(row_ids.tolist())}
    for ht in hts:
        got = ix.search(q, k, nprobe, ht)
        qcodes = ix.last_query_codes()
        assert qcodes.shape == (len(q), probes.shape[1], M) and np.array_equal(ix.last_probes(), probes)
        w_ids, w_dist, w_cnt, passed = ref.filter_answer(all_ids, all_dist, all_cnt, row_of, codes, cells, probes, qcodes, ht, k)
        _same(got, (w_ids, w_dist, w_cnt), f"ht = {ht}")
        assert ix.last_ht_stats()["rows_scored"] == passed, f"ht = {ht}: rows_scored"
        assert ix.last_stats()["rows_scanned"] == plain_stats["rows_scanned"], "rows_scanned is that of the plain search"
        print(f"M={M} ht={ht}: {passed} of {plain_stats['rows_scanned']} rows scored, counts {w_cnt.min()}..{w_cnt.max()}")
        if ht == 1:  # only rows whose code IS the query code
            for qi in range(len(q)):
                for i in got[0][qi, :got[2][qi]].tolist():
                    j = probes[qi].tolist().index(int(cells[row_of[i]]))
                    assert np.array_equal(codes[row_of[i]], qcodes[qi, j])
        if ht >= 8 * M + 1:
            assert passed == plain_stats["rows_scanned"]
            _same(got, plain, "ht = 8M + 1 against the unfiltered search")
    for ht in (0, -3):
        _same(ix.search(q, k, nprobe, ht), plain, f"ht = {ht} against the unfiltered search")
        assert ix.last_ht_stats()["rows_scored"] == ix.last_stats()["rows_scanned"] == plain_stats["rows_scanned"]
    return probes, qcodes


# ---- 1. the filter, exactly ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nq", [5, 33])
def test_filter_is_exact(pkg, built, metric, nq):
    ix, x, q, ids = built("m8", metric)
    assert ix.is_polysemous
    _check_filter(pkg, ix, q[:nq], ids, 10, SHAPES["m8"][4], [1, 16, 32, 65])


@pytest.mark.parametrize("metric", METRICS)
def test_a_stored_row_as_query_meets_its_own_code(pkg, built, metric):
    """The query code is the encoding by the index's own encoder rule: a query that is a stored row has, in the row's cell,
    the row's code, so ht = 1 (equal codes only) still finds the row."""
    ix, x, q, ids = built("m8", metric)
    got_ids, _, cnt = ix.search(x[:40], 10, 1, 1)
    codes, cells = ix.codes(), ix.assignment()[1]
    assert np.array_equal(ix.last_probes()[:, 0], cells[:40]), "a stored row probes its own cell first"
    assert np.array_equal(ix.last_query_codes()[:, 0, :], codes[:40])
    for i in range(40):
        assert cnt[i] >= 1 and ids[i] in got_ids[i, :cnt[i]].tolist()


# ---- 2. the query codes ---------------------------------------------------------------------------------------------------
def _query_code_margins(metric, q, cent, cb, probes, qcodes=None):
    """float64 ||fl32(q16 - c)_m - cb[m][j]||^2 of every (pair, subspace): the arg-min, whether it is unique by more than
    1e-5 relative + 1e-7 absolute, and (with qcodes) the distance of the chosen codeword and the minimum."""
    mi = REF_METRIC[metric]
    qp, cp = pq.prepare(mi, q), np.asarray(cent, np.float32)
    nq, nprobe = probes.shape
    res = (qp[:, None, :] - cp[probes]).reshape(nq * nprobe, -1)  # float32 subtraction of the stored values
    dist = pq.sub_distances(res, cb)  # [pairs, M, 256]
    part = np.partition(dist, 1, axis=2)
    best, second = part[:, :, 0], part[:, :, 1]
    margin = 1e-5 * best + 1e-7
    clear = second - best > margin
    chosen = None
    if qcodes is not None:
        chosen = np.take_along_axis(dist, qcodes.reshape(nq * nprobe, -1, 1).astype(np.int64), axis=2)[:, :, 0]
    return np.argmin(dist, axis=2), clear, best, margin, chosen


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", ["m8", "m48"])
def test_query_codes_are_the_encoding_of_the_residual(pkg, built, shape, metric):
    ix, x, q, ids = built(shape, metric)
    nprobe = 3
    ix.search(q, 10, nprobe, 4 * ix.M)
    probes, qcodes = ix.last_probes(), ix.last_query_codes()
    arg, clear, best, margin, chosen = _query_code_margins(metric, q, ix.centroids(), ix.codebooks(), probes, qcodes)
    unclear = 1.0 - clear.mean()
    print(f"{shape} {metric}: {unclear:.5f} of {clear.size} (pair, subspace) entries within the margin")
    assert unclear <= 0.01, "too many entries left to the margin: the comparison would be vacuous"
    assert np.all(chosen - best <= margin), "the chosen codeword is a nearest one"
    got = qcodes.reshape(arg.shape)
    assert np.array_equal(got[clear], arg[clear].astype(np.uint8)), "and the arg-min where that is unique"


# ---- 3. other code widths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", ["m4", "m48", "m64"])
def test_other_code_widths(pkg, built, shape, metric):
    d, M, nlist, n, nprobe = SHAPES[shape]
    ix, x, q, ids = built(shape, metric)
    _check_filter(pkg, ix, q[:33], ids, 10, nprobe, [1, 2 * M, 4 * M, 8 * M + 1])


# ---- 4. fallback rounds -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_fallback_rounds(pkg, metric):
    """Two lists of 20000 rows in all, both probed: more than the 8192-survivor buffer holds, so the scan runs again with a
    threshold.  ht = 8M rejects only a code that is the query code's complement.  The restatement takes the device's own
    distances from unfiltered searches of twin indexes that hold 1000 of the rows each (a distance is a function of the
    centroids, codebooks, code, probe and query), filters them by the exported codes, and sorts by (distance, id)."""
    m = _metric(pkg, metric)
    d, M, nlist, n, nq, k = 32, 8, 2, 20000, 5, 10
    rng = np.random.default_rng(77 + METRICS.index(metric))
    x = rng.standard_normal((n + nq, d)).astype(np.float32)
    x, q = x[:n], x[n:]
    ids = rng.permutation(n).astype(np.int64) * 3 + 1
    cent = x[:nlist].copy()
    cb = np.ascontiguousarray((x[100:356] - cent[0]).reshape(256, M, d // M).transpose(1, 0, 2), np.float32)
    ix = pkg.polysemous_ann.PolysemousIvfPq.adopt(pkg.ivfpq_ann.FaissIvfPq.load(m, cent, cb))
    ix.add(x, ids)
    got = ix.search(q, k, 2, 8 * M)
    assert ix.last_stats()["rounds"] >= 2, "the survivor buffer overflowed"
    probes, qcodes, codes, cells = ix.last_probes(), ix.last_query_codes(), ix.codes(), ix.assignment()[1]
    cand_ids, cand_dist = [[] for _ in range(nq)], [[] for _ in range(nq)]
    for r0 in range(0, n, 1000):
        twin = pkg.ivfpq_ann.FaissIvfPq.load(m, cent, cb)
        twin.add(x[r0:r0 + 1000], ids[r0:r0 + 1000])
        assert np.array_equal(twin.codes(), codes[r0:r0 + 1000]) and np.array_equal(twin.assignment()[1], cells[r0:r0 + 1000])
        t_ids, t_dist, t_cnt = twin.search(q, 1024, 2)
        assert np.array_equal(twin.last_probes(), probes) and np.all(t_cnt == 1000)
        twin.close()
        for qi in range(nq):
            cand_ids[qi].append(t_ids[qi, :1000])
            cand_dist[qi].append(t_dist[qi, :1000])
    row_of = {int(i): r for r, i in enumerate(ids.tolist())}
    passed = 0
    for qi in range(nq):
        c_ids, c_dist = np.concatenate(cand_ids[qi]), np.concatenate(cand_dist[qi])
        rows = np.array([row_of[i] for i in c_ids.tolist()])
        slot = np.where(cells[rows] == probes[qi, 0], 0, 1)
        ham = ref._POP[codes[rows] ^ qcodes[qi][slot]].sum(axis=1)
        keep = ham < 8 * M
        passed += int(keep.sum())
        order = np.lexsort((c_ids[keep], c_dist[keep]))[:k]
        assert got[2][qi] == k
        assert np.array_equal(got[0][qi], c_ids[keep][order]), f"query {qi}: ids"
        assert got[1][qi].tobytes() == c_dist[keep][order].tobytes(), f"query {qi}: distance bits"
    assert ix.last_ht_stats()["rows_scored"] == passed and ix.last_stats()["rows_scanned"] == n * nq
    ix.close()


# ---- 5. training ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_training(pkg, built, metric):
    ps = pkg.polysemous_ann
    d, M, nlist, n, nprobe = SHAPES["m8"]
    ix, x, q, ids = built("m8", metric)
    again = ps.PolysemousIvfPq.train(_metric(pkg, metric), nlist, M, x, niter=3, seed=5, anneal_iters=ANNEAL)
    plain = pkg.ivfpq_ann.FaissIvfPq.train(_metric(pkg, metric), nlist, M, x, niter=3, seed=5)
    assert again.codebooks().tobytes() == ix.codebooks().tobytes(), "two trainings, identical codebooks"
    assert again.centroids().tobytes() == ix.centroids().tobytes() == plain.centroids().tobytes(), "the centroids of ivfpq_index_train"
    plain_cb = plain.codebooks()
    perms = np.stack([ps.optimize_codebook(plain_cb[mm], ANNEAL, ps.subspace_seed(5, mm))[0] for mm in range(M)])
    assert any(p.tolist() != list(range(256)) for p in perms), "the annealing moved something"
    assert ps.renumber(plain_cb, perms).tobytes() == ix.codebooks().tobytes(), "the plain codebooks under the permutations"
    assert again.is_polysemous and ix.is_polysemous and again.n == 0
    plain = ps.adopt(plain)
    assert not plain.is_polysemous
    again.close()
    plain.close()


# ---- 6. OPQ ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_opq(pkg, metric):
    ps = pkg.polysemous_ann
    m = _metric(pkg, metric)
    rng = np.random.default_rng(60 + METRICS.index(metric))
    centres = rng.standard_normal((8, 40)) * 0.7
    x = (centres[rng.integers(0, 8, 2033)] + rng.standard_normal((2033, 40))).astype(np.float32)
    x, q = x[:2000], x[2000:]
    ids = rng.permutation(2000).astype(np.int64) * 5 + 2
    spec = ps.index_factory(40, "OPQ8_32,IVF8,PQ8", m)
    ix = spec.train(x, 3, 5, niter_opq=2, anneal_iters=ANNEAL)
    assert isinstance(ix, ps.PolysemousOpqIvfPq) and ix.is_polysemous and (ix.d_in, ix.d_out, ix.M) == (40, 32, 8)
    ix.add(x, ids)
    _check_filter(pkg, ix, q, ids, 10, 2, [16, 65])
    # the np string trains plain codes: the matrix, the centroids and the flag say so
    plain = ps.index_factory(40, "OPQ8_32,IVF8,PQ8np", m).train(x, 3, 5, niter_opq=2)
    assert not plain.is_polysemous and plain.matrix().tobytes() == ix.matrix().tobytes()
    assert plain.centroids().tobytes() == ix.centroids().tobytes() and plain.codebooks().tobytes() != ix.codebooks().tobytes()
    plain.close()
    ix.close()


# ---- 7. files ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["L2", "Cosine"])
def test_saved_index_answers_the_same(pkg, built, metric, tmp_path):
    ff, ps = pkg.faiss_files, pkg.polysemous_ann
    ix, x, q, ids = built("m8", metric)
    before = [ix.search(q, 10, 2, ht) for ht in (16, 24)]
    codes_before = ix.last_query_codes()
    ff.write_index(ix, tmp_path / "ix")
    loaded = ps.adopt(ff.load_native_index(32, _metric(pkg, metric), tmp_path / "ix"))
    assert isinstance(loaded, ps.PolysemousIvfPq) and not loaded.is_polysemous, "polysemous in all but the flag"
    assert loaded.codebooks().tobytes() == ix.codebooks().tobytes()
    for ht, want in zip((16, 24), before):
        _same(loaded.search(q, 10, 2, ht), want, f"loaded, ht = {ht}")
    assert np.array_equal(loaded.last_query_codes(), codes_before)
    loaded.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_index_usable(pkg):
    ps = pkg.polysemous_ann
    lib = ps._lib()
    x, q, ids = _data("m8", "L2")
    rng = np.random.default_rng(3)
    cb = (rng.integers(-32, 33, (8, 256, 4)) / 64.0).astype(np.float32)
    ix = ps.PolysemousIvfPq.adopt(pkg.ivfpq_ann.FaissIvfPq.load(_metric(pkg, "L2"), x[:8], cb))
    ix.add(x, ids)
    nq32, np32 = C.c_int32(), C.c_int32()
    assert lib.ivfpq_last_query_codes(ix._h, C.byref(nq32), C.byref(np32), None) == EINVAL
    assert b"ht > 0" in lib.ivfpq_last_error()
    with pytest.raises(ps.PolysemousError, match="no query codes"):
        ix.last_query_codes()
    ix.search(q, 10, 2, 0)  # ht <= 0 is the plain search: still no query codes
    assert lib.ivfpq_last_query_codes(ix._h, None, None, None) == EINVAL
    before = ix.search(q, 10, 2, 20)
    codes = ix.last_query_codes()
    dist, oid, cnt = np.zeros((33, 10), np.float32), np.zeros((33, 10), np.int64), np.zeros(33, np.int32)

    def call(nq=33, qp=q.ctypes.data, k=10, nprobe=2, ht=20, a=dist.ctypes.data, b=oid.ctypes.data, c=cnt.ctypes.data):
        return lib.ivfpq_search_ht(ix._h, nq, qp, k, nprobe, ht, a, b, c), lib.ivfpq_last_error()

    plain_lib = pkg.ivfpq_ann._lib()
    for kw, word in [(dict(a=None), b"null"), (dict(b=None), b"null"), (dict(c=None), b"null"), (dict(qp=None), b"null"),
                     (dict(k=0), b"k must"), (dict(k=1025), b"k must"), (dict(nprobe=0), b"nprobe"), (dict(nprobe=1025), b"nprobe"),
                     (dict(nq=0), b"nq")]:
        for ht in (20, 0):
            rc, msg = call(ht=ht, **kw)
            assert rc == EINVAL and word in msg, (kw, ht, msg)
    assert plain_lib.ivfpq_search(ix._h, 33, q.ctypes.data, 1025, 2, dist.ctypes.data, oid.ctypes.data, cnt.ctypes.data) == EINVAL
    assert np.array_equal(ix.last_query_codes(), codes), "a refused call leaves the last filtered search's codes"
    _same(ix.search(q, 10, 2, 20), before, "the index stays usable")
    assert ix.search(q, 10, 100, 20)[2].max() <= 10 and ix.last_query_codes().shape == (33, 8, 8), "nprobe is clamped to nlist"
    # an empty index has query codes and no rows
    empty = ps.PolysemousIvfPq.adopt(pkg.ivfpq_ann.FaissIvfPq.load(_metric(pkg, "L2"), x[:8], cb))
    e_ids, e_dist, e_cnt = empty.search(q, 10, 2, 20)
    assert not e_cnt.any() and not e_ids.any() and empty.last_ht_stats()["rows_scored"] == 0
    ix.search(q, 10, 2, 20)
    assert np.array_equal(empty.last_query_codes(), ix.last_query_codes()), "the query code needs no row"
    empty.close()
    ix.close()


# ---- 9. existing behaviour ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ivfpq", "opq"])
def test_plain_searches_answer_as_before_the_filter(pkg, kind):
    """ivfpq_search / opq_search byte for byte against tests/golden/*_search_baseline.npz, as tests/test_refine_gpu.py
    loads them: the filtered scan is an instantiation beside the existing one."""
    path = os.path.join(ROOT, "tests", "golden", "make_pq_search_baseline.py")
    spec = importlib.util.spec_from_file_location("make_pq_search_baseline", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = np.load(os.path.join(ROOT, "tests", "golden", f"{kind}_search_baseline.npz"))
    got = gen.answers(pkg, kind)
    assert sorted(got) == sorted(want.files) and len(got) == 3 * len(gen.METRICS) * len(gen.SEARCHES)
    for name in sorted(got):
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), name


def test_filtered_search_answers_as_before_the_shared_core(pkg):
    """search(q, 10, 4, ht) of an adopted ivfpq index at a threshold where the filter both drops and keeps rows, with
    last_query_codes() and the rows scored and scanned, byte for byte against what the library gave before ivf_ann.hip and
    ivfpq_ann.hip shared csrc/ivf_core.h (tests/golden/ivf_family_baseline.npz, written by make_ivf_family_baseline.py)."""
    path = os.path.join(ROOT, "tests", "golden", "make_ivf_family_baseline.py")
    spec = importlib.util.spec_from_file_location("make_ivf_family_baseline", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    base = np.load(os.path.join(ROOT, "tests", "golden", "ivf_family_baseline.npz"))
    want = {n: base[n] for n in base.files if n.startswith("ht_")}
    got = gen.ht_answers(pkg)
    assert sorted(got) == sorted(want) and len(got) == 6 * len(gen.METRICS) + 1
    for name in sorted(got):
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), name
    assert any(want[n].any() for n in want if n.endswith("_dist"))
