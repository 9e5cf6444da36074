"""The OPQ pre-transform on the device (include/opq_ann.h) against the restatements tests/_opq_ref.py (the transform, the
correlation) and tests/_ivfpq_ref.py (everything behind the transform, fed with what the index exports and with the
device's own opq_transform of the queries -- never with the device's distances).
PARITY UNPINNED against Faiss's OPQMatrix::train (not vendored in the reference), as the header says.

Bounds.  Transform: a component's fp32 FMA chain of d_in terms against float64, (d_in + 1) 2^-24 sum_i |A_ji x_i|; Cosine
3 2^-24 |y| more for the fp32 norm.  Correlation: n 2^-52 sum |x_i y^_j| per entry (fp64 sums of n exact products, by
chunk).  Search: the tolerances, the unclear-position rule and the cap (0.15) of tests/test_ivfpq_gpu.py.

Search parity through a projection takes the _low_dimensional rows of tests/test_ivfpq_gpu.py (copied below), 40 -> 32 under
a random orthonormal matrix, n = 3000, nq = 33, k = 10, M = 8, nlist = 8.  Computed from the restatements alone (no device:
centroids 8 rows and codebooks the residual pieces of 256 rows picked at random, as niter = -1 gives them), the share of
unclear positions for the data seed used here is, at nprobe = 1 and 8: L2 0.000 and 0.000, Cosine 0.015 and 0.015,
InnerProduct 0.024 and 0.036 -- far under the cap.

Training does its job: rows of 32 components with sigma = 1 in the first 4 (= dsub at M = 8) and 0.02 elsewhere, seed 21.
From the restatement alone (_opq_ref.pq_numpy, 256 codewords per subspace, 10 Lloyd rounds, 4096 rows): the mean squared
quantisation error ||y - y^||^2 is 0.3113 for the rows as they are -- one sub-quantizer carries all of the variance --
and 0.1322 for the rows under a random rotation (seed 22), which spreads it over the 8 sub-quantizers."""
import ctypes as C

import numpy as np
import pytest

import _ivfpq_ref as pqref
import _opq_ref as ref

pytestmark = pytest.mark.gpu

METRICS = ["L2", "Cosine", "InnerProduct"]
MAX_UNCLEAR = 0.15
EINVAL = 1


def _metric(pkg, name):
    return getattr(pkg.dense_ann.DistanceMetric, name)


def _low_dimensional(rng, n, d, r=3, eps=0.3):
    """N(0,1) latent rows of dimension r under a random N(0,1) / sqrt(r) linear map into R^d, plus eps N(0,1) per component:
    distances that spread instead of concentrating (see the docstring of tests/test_ivfpq_gpu.py)."""
    basis = rng.standard_normal((r, d)) / np.sqrt(r)
    return (rng.standard_normal((n, r)) @ basis + eps * rng.standard_normal((n, d))).astype(np.float32)


def _orthonormal(rng, d_out, d_in):
    q, _ = np.linalg.qr(rng.standard_normal((d_in, d_out)))
    return np.ascontiguousarray(q.T, np.float32)


def _transformer(pkg, metric, A):
    """An index that is only its matrix: one all-zero cell, all-zero codebooks."""
    d_out = A.shape[0]
    return pkg.opq_ann.FaissOpqIvfPq.load(metric, A, np.zeros((1, d_out), np.float32), np.zeros((4, 256, d_out // 4), np.float32))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. the transform -------------------------------------------------------------------------------------------------
SHAPES = [(16, 16), (40, 32), (512, 512)]


@pytest.mark.parametrize("metric", ["L2", "Cosine"])
@pytest.mark.parametrize("d_in,d_out", SHAPES)
def test_transform_against_float64(pkg, metric, d_in, d_out):
    m = _metric(pkg, metric)
    rng = np.random.default_rng(1000 + d_in)
    A = rng.standard_normal((d_out, d_in)).astype(np.float32)
    ix = _transformer(pkg, m, A)
    assert np.array_equal(ix.matrix(), A), "the matrix is kept as given"
    for n in [1, 63, 65, 1000] + ([130] if d_in == 512 else []):
        x = (rng.standard_normal((n, d_in)) * np.exp(rng.standard_normal((n, 1)))).astype(np.float32)
        got = ix.transform(x)
        assert got.shape == (n, d_out) and got.dtype == np.float32
        want, S = ref.transform(int(m), A, x)
        err = np.abs(got.astype(np.float64) - want)
        bound = ref.transform_bound(int(m), d_in, S, want)
        print(f"{metric} {d_in}->{d_out} n={n}: worst error / bound {np.max(err / bound):.4f}")
        assert np.all(err <= bound)
    ix.close()


@pytest.mark.parametrize("d_in,d_out", SHAPES)
def test_a_signed_permutation_moves_the_bits(pkg, d_in, d_out):
    rng = np.random.default_rng(1100 + d_in)
    perm = rng.permutation(d_in)[:d_out]
    sign = rng.choice([-1.0, 1.0], d_out).astype(np.float32)
    A = np.zeros((d_out, d_in), np.float32)
    A[np.arange(d_out), perm] = sign
    ix = _transformer(pkg, _metric(pkg, "InnerProduct"), A)
    x = rng.standard_normal((333, d_in)).astype(np.float32)
    assert np.all(x != 0)
    assert np.array_equal(_bits(ix.transform(x)), _bits(x[:, perm] * sign[None, :]))
    ix.close()


@pytest.mark.parametrize("metric", ["L2", "Cosine"])
@pytest.mark.parametrize("d_in,d_out", SHAPES)
def test_a_row_does_not_depend_on_its_batch(pkg, metric, d_in, d_out):
    rng = np.random.default_rng(1200 + d_in)
    ix = _transformer(pkg, _metric(pkg, metric), rng.standard_normal((d_out, d_in)).astype(np.float32))
    x = rng.standard_normal((200, d_in)).astype(np.float32)
    row = rng.standard_normal((1, d_in)).astype(np.float32)
    alone = _bits(ix.transform(row))
    for at in (0, 199, 77):
        batch = x.copy()
        batch[at] = row[0]
        assert np.array_equal(_bits(ix.transform(batch)[at:at + 1]), alone), f"position {at} of 200"
    assert np.array_equal(_bits(ix.transform(np.concatenate([x[:64], row]))[64:]), alone), "first row of a second tile"
    ix.close()


# ---- 2. the identity seam ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_the_identity_matrix_gives_the_plain_index(pkg, metric):
    m = _metric(pkg, metric)
    rng = np.random.default_rng(20)
    n, d, M, nlist = 3000, 32, 8, 8
    x = _low_dimensional(rng, n + 33, d)
    x, q = x[:n], x[n:]
    ids = rng.permutation(n).astype(np.int64) * 3 + 5
    trained = pkg.ivfpq_ann.FaissIvfPq.train(m, nlist, M, x[:1000], niter=2, seed=3)
    cent, cb = trained.centroids(), trained.codebooks()
    trained.close()
    plain = pkg.ivfpq_ann.FaissIvfPq.load(m, cent, cb)
    # Cosine: the plain index normalises the centroids it is given and the inner index (InnerProduct) does not, so the
    # OPQ index is loaded with the centroids the plain index stores: the same centroids in both
    opq = pkg.opq_ann.FaissOpqIvfPq.load(m, np.eye(d, dtype=np.float32), plain.centroids(), cb)
    assert np.array_equal(opq.centroids(), plain.centroids()) and np.array_equal(opq.codebooks(), plain.codebooks())
    plain.add(x, ids)
    opq.add(x[:1700], ids[:1700])
    opq.add(x[1700:], ids[1700:])
    assert opq.n == n
    assert np.array_equal(opq.codes(), plain.codes())
    for a, b in zip(opq.assignment(), plain.assignment()):
        assert np.array_equal(a, b)
    assert np.array_equal(opq.list_sizes(), plain.list_sizes())
    for nprobe in (1, 8):
        o_ids, o_dist, o_cnt = opq.search(q, 10, nprobe)
        p_ids, p_dist, p_cnt = plain.search(q, 10, nprobe)
        assert np.array_equal(opq.last_probes(), plain.last_probes())
        assert np.array_equal(o_cnt, p_cnt) and np.array_equal(o_ids, p_ids)
        if metric == "Cosine":
            assert np.all(np.abs(o_dist.astype(np.float64) - p_dist) <= pqref.ATOL + pqref.RTOL * np.abs(p_dist))
        else:
            assert np.array_equal(_bits(o_dist), _bits(p_dist))
        st = opq.last_stats()
        assert st["rows_scanned"] == plain.last_stats()["rows_scanned"] and st["transform_ms"] > 0
    plain.close()
    opq.close()


# ---- 3. search parity through a projection ----------------------------------------------------------------------------
def _compare(ix, metric, got, want, k):
    """tests/test_ivfpq_gpu.py's _compare: got = (ids, dist, cnt) against want (ids, values, S per query).  metric is the
    inner metric.  Returns (unclear, total)."""
    got_ids, got_dist, cnt = got
    M, dsub = ix.M, ix.d // ix.M
    unclear = total = 0
    for q, (r_ids, r_val, r_s) in enumerate(want):
        m = min(k, len(r_ids))
        assert cnt[q] == m, f"query {q}: count {cnt[q]} != {m}"
        if m == 0:
            continue
        tol = pqref.tolerance(metric, r_val, r_s, M, dsub)
        g = got_dist[q, :m].astype(np.float64)
        g = g * g if metric == pqref.L2 else g
        err = np.abs(g - r_val[:m])
        assert np.all(err <= tol[:m]), f"query {q}: error {err.max()} against tolerance {tol[:m][err.argmax()]}"
        assert np.all(np.diff(got_dist[q, :m]) >= 0), "ascending"
        nxt = r_val[m] if len(r_val) > m else np.inf
        clear = pqref.clear_positions(r_val[:m], nxt, tol[:m])
        assert np.array_equal(got_ids[q, :m][clear], r_ids[:m][clear])
        assert len(set(got_ids[q, :m].tolist())) == m, "no id twice"
        unclear += int((~clear).sum())
        total += m
    return unclear, total


@pytest.mark.parametrize("metric", METRICS)
def test_search_through_a_projection_matches_the_restatement(pkg, metric):
    m = _metric(pkg, metric)
    inner = ref.inner_metric(int(m))
    rng = np.random.default_rng(30)
    n, d_in, d_out, M, nlist, nq, k = 3000, 40, 32, 8, 8, 33, 10
    x = _low_dimensional(rng, n + nq, d_in)
    x, q = x[:n], x[n:]
    ids = rng.permutation(n).astype(np.int64) * 5 + 2
    A = _orthonormal(rng, d_out, d_in)
    # cells and codebooks of the transformed rows (computed here in float32: they only have to be sensible)
    y = (ref.prepare(int(m), x) @ A.T.astype(np.float64)).astype(np.float32)
    trained = pkg.ivfpq_ann.FaissIvfPq.train(pkg.dense_ann.DistanceMetric(inner), nlist, M, y[:1000], niter=-1, seed=6)
    ix = pkg.opq_ann.FaissOpqIvfPq.load(m, A, trained.centroids(), trained.codebooks())
    trained.close()
    ix.add(x, ids)
    got_ids, cells = ix.assignment()
    assert np.array_equal(got_ids, ids) and ix.list_sizes().sum() == n
    for nprobe in (1, 8):
        got = ix.search(q, k, nprobe)
        want = pqref.adc_search(inner, ix.centroids(), ix.codebooks(), ix.codes(), ids, cells, ix.last_probes(),
                                pqref.prepare(inner, ix.transform(q)), k)
        unclear, total = _compare(ix, inner, got, want, k)
        print(f"{metric} nprobe={nprobe}: unclear positions {unclear / max(total, 1):.4f} of {total}")
        assert unclear <= MAX_UNCLEAR * total, "the comparison would be vacuous"
    info = [C.c_int32() for _ in range(5)]
    lib = pkg.opq_ann._lib()
    assert lib.opq_index_info(ix._h, None, *[C.byref(v) for v in info]) == 0
    assert [v.value for v in info] == [d_in, d_out, int(m), nlist, M], "the outer metric is reported"
    ix.close()


# ---- 4. the correlation -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, 5000])
def test_correlation_against_float64(pkg, n):
    rng = np.random.default_rng(40 + n)
    x = rng.standard_normal((n, 40)).astype(np.float32)
    y = rng.standard_normal((n, 32)).astype(np.float32)
    got = pkg.opq_ann.debug_correlation(x, y)
    want, S = ref.correlation(x, y)
    err = np.abs(got - want)
    bound = n * 2.0 ** -52 * S
    print(f"n={n}: worst error / bound {np.max(err / bound):.4f}")
    assert got.shape == (40, 32) and np.all(err <= bound)
    assert pkg.opq_ann.debug_correlation(x, y).tobytes() == got.tobytes(), "two runs are byte-identical"


# ---- 5. training ------------------------------------------------------------------------------------------------------
def _concentrated(rng, n, d=32, hot=4):
    """Rows whose variance sits in the first `hot` components: sigma = 1 there and 0.02 elsewhere."""
    x = 0.02 * rng.standard_normal((n, d))
    x[:, :hot] = rng.standard_normal((n, hot))
    return x.astype(np.float32)


def test_training_is_deterministic_and_lowers_the_error(pkg):
    m = _metric(pkg, "L2")
    x = _concentrated(np.random.default_rng(21), 4096)
    a = pkg.opq_ann.FaissOpqIvfPq.train(m, 8, 8, 32, x, niter=2, niter_opq=8, seed=7)
    b = pkg.opq_ann.FaissOpqIvfPq.train(m, 8, 8, 32, x, niter=2, niter_opq=8, seed=7)
    A = a.matrix()
    assert A.shape == (32, 32) and np.all(np.isfinite(A))
    assert np.abs(A @ A.T - np.eye(32, dtype=np.float32)).max() <= 1e-5, "orthonormal in fp32"
    assert A.tobytes() == b.matrix().tobytes()
    assert a.centroids().tobytes() == b.centroids().tobytes()
    assert a.codebooks().tobytes() == b.codebooks().tobytes()
    err = a.training_errors()
    print("training errors", err.tolist(), a.training_stats())
    assert err.shape == (8,) and np.all(np.isfinite(err)) and err[7] < err[0]
    assert err.tobytes() == b.training_errors().tobytes()
    a.close()
    b.close()


def test_training_does_its_job(pkg):
    m = _metric(pkg, "L2")
    rng = np.random.default_rng(21)
    n, nlist, M = 4096, 8, 8
    x = _concentrated(rng, n + 200)
    x, q = x[:n], x[n:]
    opq = pkg.opq_ann.FaissOpqIvfPq.train(m, nlist, M, 32, x, niter=5, niter_opq=8, seed=7)
    plain = pkg.ivfpq_ann.FaissIvfPq.train(m, nlist, M, x, niter=5, seed=7)
    mse = {}
    for name, ix in (("opq", opq), ("plain", plain)):
        ix.add(x)
        ids, dist, cnt = ix.search(q, 1, nlist)
        assert np.all(cnt == 1)
        exact = np.sqrt(((x[ids[:, 0]].astype(np.float64) - q.astype(np.float64)) ** 2).sum(axis=1))
        mse[name] = float(np.mean((dist[:, 0].astype(np.float64) - exact) ** 2))
        ix.close()
    print("mean squared difference between reported and exact distance", mse)
    assert mse["opq"] < mse["plain"]


# ---- 6. errors --------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_with_a_message(pkg):
    lib = pkg.opq_ann._lib()
    h = C.c_void_p()
    x = np.zeros((300, 1040), np.float32)

    def train(d_in=32, d_out=32, nlist=8, M=8, n=300, niter_opq=1):
        rc = lib.opq_index_train(0, 0, d_in, d_out, nlist, M, n, x.ctypes.data, 1, niter_opq, 1, C.byref(h))
        return rc, lib.opq_last_error().decode()

    for kw, what in [(dict(d_in=32, d_out=48), "d_out"), (dict(d_out=32, M=12), "divide"), (dict(d_out=24, d_in=24), "multiple of 16"),
                     (dict(d_in=1040), "d_in"), (dict(niter_opq=-1), "niter_opq"), (dict(n=255), "n_train"),
                     (dict(n=300, nlist=301), "n_train")]:
        rc, msg = train(**kw)
        assert rc == EINVAL and what in msg, (kw, msg)
    cent, cb = np.zeros((8, 32), np.float32), np.zeros((8, 256, 4), np.float32)
    assert lib.opq_index_load(0, 0, 32, 32, 8, 8, None, cent.ctypes.data, cb.ctypes.data, C.byref(h)) == EINVAL
    assert "null" in lib.opq_last_error().decode()
    assert h.value is None
    # the device is as it was
    ix = _transformer(pkg, _metric(pkg, "L2"), np.eye(16, dtype=np.float32))
    v = np.arange(32, dtype=np.float32).reshape(2, 16) + 1
    assert np.array_equal(ix.transform(v), v)
    with pytest.raises(pkg.opq_ann.OpqError, match="k must"):
        ix.search(v, 1025, 1)
    with pytest.raises(ValueError):
        ix.add(np.zeros((2, 17), np.float32))
    ix.close()


# ---- 7. the mirror, end to end ----------------------------------------------------------------------------------------
def test_build_faiss_index_end_to_end(pkg):
    oq = pkg.opq_ann
    m = _metric(pkg, "Cosine")
    rng = np.random.default_rng(50)
    v = _low_dimensional(rng, 2000, 40)
    ids = rng.permutation(2000).astype(np.int64) * 11 + 1000
    ix = oq.build_faiss_index(v, ids, 1.0, "OPQ8_32,IVF8,PQ8", m, niter=2, niter_opq=2)
    assert isinstance(ix, oq.FaissOpqIvfPq) and (ix.n, ix.d_in, ix.d_out, ix.M, ix.nlist) == (2000, 40, 32, 8, 8)
    k = 10
    got_ids, dist, cnt = ix.search(v[:50], k, 4)
    known = set(ids.tolist())
    for qi in range(50):
        c = cnt[qi]
        assert 0 < c <= k and set(got_ids[qi, :c].tolist()) <= known
        pairs = list(zip(dist[qi, :c].tolist(), got_ids[qi, :c].tolist()))
        assert pairs == sorted(pairs), "ascending by (distance, id)"
    got = pkg.ivf_ann.FaissQueryable(ix, m).queryWithDistance(v[17], 5, pkg.ivf_ann.FaissParams(nprobe=4))
    assert [i for i, _ in got] == got_ids[17, :5].tolist()
    ix.close()
