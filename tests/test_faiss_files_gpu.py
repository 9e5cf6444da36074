"""Save -> load of the three inverted-file indexes (include/faiss_files.h) on the device: a loaded index is the saved one,
bit for bit.  Every comparison is an equality of bytes or of an exact composition (dann_compose_shards), so no tolerance is
chosen anywhere.

Shapes: d = 32, nlist = 8, M = 8, 600 rows, 5 queries, k = 10, nprobe = 3; OPQ 40 -> 32.  The indexes of the identity tests
are built from given centroids (`*_load`) with rows placed around them, so that the lists hold 0, 64 (one full block of the
PQ scan), 200 (more than one block), 100, 80, 60, 50 and 46 rows.  The centroids are not of unit length.

What a Cosine index stores is the centroid divided by its fp32 norm and rounded to fp16.  Doing that a second time to the
stored value almost always gives the stored value back (the rounded row's norm is within about 2e-4 of 1, less than half an
fp16 ulp per component): about one random row of 32 components in 10^4 changes.  A restore that normalised again would
therefore pass a byte comparison on arbitrary centroids.  Centroids 3, 5 and 6 are rows found by search (RENORM_SEEDS) for
which the second pass does change bits; test_second_normalisation_changes_the_chosen_centroids asserts that with a numpy
restatement of the arithmetic, and the Cosine identity cases assert it on the device through `*_load`, which normalises."""
import datetime as dt
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = ["flat", "pq", "opq"]
METRICS = ["L2", "Cosine", "InnerProduct"]
D, D_IN, NLIST, M, K, NPROBE = 32, 40, 8, 8, 10, 3
SIZES = [0, 64, 200, 100, 80, 60, 50, 46]
EINVAL = 1
UTC = dt.timezone.utc
# centroid -> seed of the N(0,1) draw that replaces its noise: found by searching seeds 100000, 100001, ... for rows that the
# second normalise-and-round pass changes
RENORM_SEEDS = {3: 131228, 5: 100193, 6: 101945}


def _normalise_and_round(x):
    """prep_rows_kernel / store_rows_kernel with normalise = 1: fp64 sum of squares, fp32 norm, fp32 divide, fp16."""
    x = np.asarray(x, np.float32)
    norm = np.sqrt((x.astype(np.float64) ** 2).sum(1)).astype(np.float32)
    norm[~(norm > 0)] = 1
    return (x / norm[:, None]).astype(np.float16)


def _metric(pkg, name):
    return getattr(pkg.dense_ann.DistanceMetric, name)


@pytest.fixture(scope="module")
def data():
    """centroids [8, 32]; rows [700, 32] around them (600 by SIZES in a shuffled order, then 100 more); the same rows lifted
    to 40 dimensions through A^T (A [32, 40], orthonormal rows), so that A x gives them back; queries; PQ codebooks."""
    rng = np.random.default_rng(7)
    cent = (4.0 * np.eye(NLIST, D) + 0.3 * rng.standard_normal((NLIST, D))).astype(np.float32)
    for c, seed in RENORM_SEEDS.items():
        cent[c] = (4.0 * np.eye(NLIST, D)[c] + 0.3 * np.random.default_rng(seed).standard_normal(D)).astype(np.float32)
    cells = rng.permutation(np.repeat(np.arange(NLIST), SIZES))
    cells = np.concatenate([cells, rng.integers(1, NLIST, 100)])
    rows = (cent[cells] + 0.1 * rng.standard_normal((700, D))).astype(np.float32)
    A = np.linalg.qr(rng.standard_normal((D_IN, D)))[0].T.astype(np.float32)
    queries = (cent[[1, 2, 3, 5, 7]] + 0.2 * rng.standard_normal((5, D))).astype(np.float32)
    return dict(cent=cent, rows=rows, rows_in=(rows @ A).astype(np.float32), A=A, q=queries, q_in=(queries @ A).astype(np.float32),
                cb=(0.1 * rng.standard_normal((M, 256, D // M))).astype(np.float32), ids=rng.permutation(10**6)[:700].astype(np.int64))


def _new(pkg, kind, metric, data):
    m = _metric(pkg, metric)
    if kind == "flat":
        return pkg.ivf_ann.FaissIvfFlat.load(m, data["cent"])
    if kind == "pq":
        return pkg.ivfpq_ann.FaissIvfPq.load(m, data["cent"], data["cb"])
    return pkg.opq_ann.FaissOpqIvfPq.load(m, data["A"], data["cent"], data["cb"])


def _rows_of(kind, data, a, b):
    return data["rows_in" if kind == "opq" else "rows"][a:b]


def _queries(kind, data):
    return data["q_in" if kind == "opq" else "q"]


def _state(pkg, ix):
    """Every array the index exports, as bytes."""
    ff = pkg.faiss_files
    ids, cells = ix.assignment()
    s = dict(n=ix.n, ids_mode=ff.ids_mode(ix), centroids=ix.centroids().tobytes(), ids=ids.tobytes(), cells=cells.tobytes(),
             sizes=ix.list_sizes().tobytes())
    if hasattr(ix, "codes"):
        s["codebooks"], s["codes"] = ix.codebooks().tobytes(), ix.codes().tobytes()
    else:
        s["rows"] = ff.stored_rows(ix).tobytes()
    if hasattr(ix, "matrix"):
        s["matrix"] = ix.matrix().tobytes()
    return s


def _answers(ix, q, k=K, nprobe=NPROBE):
    ids, dist, cnt = ix.search(q, k, nprobe)
    return dict(ids=ids.tobytes(), dist=dist.tobytes(), cnt=cnt.tobytes(), probes=ix.last_probes().tobytes(), counts=cnt.tolist())


def _same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert a[key] == b[key], key


def _dim(kind):
    return D_IN if kind == "opq" else D


def test_second_normalisation_changes_the_chosen_centroids(pkg, data):
    """The premise of the Cosine identity cases, from the restatement and on the device: the stored centroids of a Cosine
    index are not a fixed point of normalise-and-round, so a restore that normalised them again could not keep their bits."""
    once = _normalise_and_round(data["cent"])
    twice = _normalise_and_round(once.astype(np.float32))
    moved = np.flatnonzero((once.view(np.uint16) != twice.view(np.uint16)).any(1)).tolist()
    assert moved == sorted(RENORM_SEEDS)
    cos = _metric(pkg, "Cosine")
    ix = pkg.ivf_ann.FaissIvfFlat.load(cos, data["cent"])
    stored = ix.centroids()
    assert stored.astype(np.float16).tobytes() == once.tobytes()  # the device stores what the restatement says
    again = pkg.ivf_ann.FaissIvfFlat.load(cos, stored)  # the path that normalises
    differ = np.flatnonzero((again.centroids() != stored).any(1)).tolist()
    assert differ == sorted(RENORM_SEEDS)
    ix.close()
    again.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", KINDS)
def test_identity_after_a_round_trip(pkg, tmp_path, data, kind, metric):
    ff = pkg.faiss_files
    ix = _new(pkg, kind, metric, data)
    ix.add(_rows_of(kind, data, 0, 600), data["ids"][:600])
    assert ix.list_sizes().tolist() == SIZES  # an empty list, one of exactly 64 rows, one of more
    ff.write_index(ix, tmp_path / "idx")
    assert sorted(os.listdir(tmp_path / "idx")) == ["_SUCCESS", "faiss.index"]
    assert os.path.getsize(tmp_path / "idx" / "_SUCCESS") == 0 and ff.is_valid_faiss_index(tmp_path / "idx")
    q = ff.FaissIndex.load_index(_dim(kind), _metric(pkg, metric), tmp_path / "idx")
    back = q.index
    assert type(back) is type(ix) and q.metric == ix.metric
    _same(_state(pkg, ix), _state(pkg, back))
    if metric == "Cosine" and kind != "opq":  # (the inner index of a Cosine OPQ index is InnerProduct: it never normalises)
        # the comparison above has teeth: the stored centroids through the path that normalises do not keep their bits
        renorm = _new(pkg, kind, metric, dict(data, cent=ix.centroids()))
        assert renorm.centroids().tobytes() != ix.centroids().tobytes()
        renorm.close()
    want, got = _answers(ix, _queries(kind, data)), _answers(back, _queries(kind, data))
    assert min(want["counts"]) > 0
    _same(want, got)
    # the adapter over the loaded index answers as over the original
    p = pkg.ivf_ann.FaissParams(nprobe=NPROBE)
    assert q.queryWithDistance(_queries(kind, data)[0], K, p) == pkg.ivf_ann.FaissQueryable(ix, ix.metric).queryWithDistance(
        _queries(kind, data)[0], K, p)
    # a directory that holds an index is not written over
    before = (tmp_path / "idx" / "faiss.index").read_bytes()
    with pytest.raises(ff.FaissFileError, match="exists already"):
        ff.write_index(back, tmp_path / "idx")
    assert (tmp_path / "idx" / "faiss.index").read_bytes() == before
    assert sorted(os.listdir(tmp_path / "idx")) == ["_SUCCESS", "faiss.index"]
    ix.close()
    back.close()


@pytest.mark.parametrize("factory,dim", [("IVF8,Flat", D), ("IVF8,PQ8", D), ("OPQ8_32,IVF8,PQ8", D_IN)])
def test_build_and_write_then_load_is_the_built_index(pkg, tmp_path, data, factory, dim):
    """FaissIndexer.buildAndWriteFaissIndex, Cosine, trained (niter = 2): what the service loads is what build_faiss_index
    builds from the same arguments (training is deterministic)."""
    ff = pkg.faiss_files
    m = _metric(pkg, "Cosine")
    rows = data["rows_in" if dim == D_IN else "rows"][:600]
    ff.build_and_write_faiss_index(rows, data["ids"][:600], 0.5, factory, m, tmp_path / "out", niter=2, niter_opq=2, seed=3)
    ix = pkg.opq_ann.build_faiss_index(rows, data["ids"][:600], 0.5, factory, m, niter=2, niter_opq=2, seed=3)
    back = ff.FaissIndex.load_index(dim, m, tmp_path / "out").index
    _same(_state(pkg, ix), _state(pkg, back))
    q = data["q_in" if dim == D_IN else "q"]
    _same(_answers(ix, q), _answers(back, q))
    ix.close()
    back.close()


@pytest.mark.parametrize("given", [True, False], ids=["ids_given", "ids_positions"])
@pytest.mark.parametrize("kind", KINDS)
def test_add_after_load(pkg, tmp_path, data, kind, given):
    ff = pkg.faiss_files
    ix = _new(pkg, kind, "L2", data)
    ix.add(_rows_of(kind, data, 0, 600), data["ids"][:600] if given else None)
    ff.write_index(ix, tmp_path / "idx")
    back = ff.load_native_index(_dim(kind), ix.metric, tmp_path / "idx")
    assert ff.ids_mode(back) == ff.ids_mode(ix) == (ff.IDS_GIVEN if given else ff.IDS_POSITIONS)
    # an add that breaks the ids rule is refused on the loaded index exactly as on the original
    more = _rows_of(kind, data, 600, 700)
    wrong = None if given else data["ids"][600:700]
    messages = []
    for index in (ix, back):
        with pytest.raises(pkg.ivf_ann.IvfError) as e:
            index.add(more, wrong)
        messages.append(str(e.value))
    assert messages[0] == messages[1]
    for index in (ix, back):
        index.add(more, data["ids"][600:700] if given else None)
    assert back.n == 700
    _same(_state(pkg, ix), _state(pkg, back))
    _same(_answers(ix, _queries(kind, data)), _answers(back, _queries(kind, data)))
    # and the grown index round-trips again
    ff.write_index(back, tmp_path / "idx2")
    again = ff.load_native_index(_dim(kind), ix.metric, tmp_path / "idx2")
    _same(_state(pkg, ix), _state(pkg, again))
    for index in (ix, back, again):
        index.close()


@pytest.mark.parametrize("kind", KINDS)
def test_empty_index(pkg, tmp_path, data, kind):
    ff = pkg.faiss_files
    ix = _new(pkg, kind, "Cosine", data)
    ff.write_index(ix, tmp_path / "idx")
    back = ff.load_native_index(_dim(kind), ix.metric, tmp_path / "idx")
    assert back.n == 0 and ff.ids_mode(back) == ff.IDS_NONE
    _same(_state(pkg, ix), _state(pkg, back))
    got = _answers(back, _queries(kind, data))
    assert got["counts"] == [0] * 5
    _same(_answers(ix, _queries(kind, data)), got)
    # it is still free to take ids or positions, as a new index is
    for index in (ix, back):
        index.add(_rows_of(kind, data, 0, 600), data["ids"][:600])
    _same(_state(pkg, ix), _state(pkg, back))
    ix.close()
    back.close()


@pytest.mark.parametrize("kind", KINDS)
def test_validation_before_layout(pkg, tmp_path, data, kind):
    """Files from the codec's writer that no checksum can fault: a cell equal to nlist; an id that is not its position in a
    file whose ids are positions.  The validation kernel refuses both, naming the row, and the device serves on."""
    ff = pkg.faiss_files
    ix = _new(pkg, kind, "L2", data)
    ix.add(_rows_of(kind, data, 0, 600), None)
    ff.write_index(ix, tmp_path / "good")
    f = ff.read_file(tmp_path / "good" / "faiss.index")
    assert f["n"] == 600 and f["ids_mode"] == ff.IDS_POSITIONS and f["ids"].tolist() == list(range(600))

    def hostile(name, **changed):
        g = dict(f, **changed)
        os.mkdir(tmp_path / name)
        ff.write_file(tmp_path / name / "faiss.index", g["kind"], g["metric"], centroids=g["centroids"], ids_mode=g["ids_mode"],
                      ids=g["ids"], cells=g["cells"], payload=g["payload"], codebooks=g.get("codebooks"), matrix=g.get("matrix"))
        (tmp_path / name / "_SUCCESS").write_bytes(b"")
        with pytest.raises(ff.FaissFileError) as e:
            ff.load_native_index(_dim(kind), ix.metric, tmp_path / name)
        assert e.value.code == EINVAL
        return e.value.message

    cells = f["cells"].copy()
    cells[437] = NLIST
    cells[512] = -1
    assert "row 437" in hostile("bad_cell", cells=cells)
    ids = f["ids"].copy()
    ids[301] = 300
    msg = hostile("bad_id", ids=ids)
    assert "row 301" in msg and "position" in msg
    back = ff.load_native_index(_dim(kind), ix.metric, tmp_path / "good")
    _same(_state(pkg, ix), _state(pkg, back))
    _same(_answers(ix, _queries(kind, data)), _answers(back, _queries(kind, data)))
    ix.close()
    back.close()


def test_dimension_or_metric_mismatch(pkg, tmp_path, data):
    ff = pkg.faiss_files
    ix = _new(pkg, "opq", "Cosine", data)
    ix.add(data["rows_in"][:600], data["ids"][:600])
    ff.write_index(ix, tmp_path / "idx")
    ix.close()
    cos, l2 = _metric(pkg, "Cosine"), _metric(pkg, "L2")
    with pytest.raises(ff.FaissFileError, match="dimension 40, not the expected 32"):
        ff.FaissIndex.load_index(D, cos, tmp_path / "idx")  # the embeddings' dimension is the transform's input
    with pytest.raises(ff.FaissFileError, match="metric"):
        ff.FaissIndex.load_index(D_IN, l2, tmp_path / "idx")
    with pytest.raises(ff.FaissFileError, match="not an index directory"):
        ff.FaissIndex.load_index(D_IN, cos, tmp_path / "absent")
    ff.FaissIndex.load_index(D_IN, cos, tmp_path / "idx").index.close()


def test_hourly_shards(pkg, tmp_path):
    ff = pkg.faiss_files
    m = _metric(pkg, "L2")
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((1200, D)).astype(np.float32)
    ids = np.arange(1200, dtype=np.int64) * 3 + 1
    q = rows[[10, 350, 620, 100, 500]] + 0.05 * rng.standard_normal((5, D)).astype(np.float32)
    now = dt.datetime(2024, 1, 1, 1, 30, tzinfo=UTC)  # the hours before cross into 2023
    root = tmp_path / "root"

    def hour_dir(back):
        return str(root / (now - dt.timedelta(hours=back)).strftime("%Y/%m/%d/%H"))

    def write(back, a, b, id_slice=None):
        os.makedirs(os.path.dirname(hour_dir(back)), exist_ok=True)
        ff.build_and_write_faiss_index(rows[a:b], ids[a:b] if id_slice is None else id_slice, 1.0, "IVF8,Flat", m, hour_dir(back),
                                       niter=2, seed=5)

    write(1, 0, 300)
    write(2, 300, 600)
    write(4, 600, 900)
    write(3, 900, 1200)
    os.unlink(os.path.join(hour_dir(3), "_SUCCESS"))  # written, but never marked complete
    sh = ff.HourlyShardedIndex(m, D, root, 3, 24)
    assert sh.reload(now) is True
    assert sh.directories == [hour_dir(1), hour_dir(2), hour_dir(4)] and sh.loads == 3 and sh.closes == 0

    def composed(dirs, k=K):
        parts = []
        for d in dirs:
            one = ff.load_native_index(D, m, d)
            parts.append(one.search(q, k, NPROBE))
            one.close()
        return pkg.dense_ann.compose(parts, k)

    def same_answers(a, b):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()

    first = sh.search(q, K, NPROBE)
    same_answers(first, composed([hour_dir(1), hour_dir(2), hour_dir(4)]))
    assert first[2].tolist() == [K] * 5
    # the same hour again: nothing is read
    assert sh.reload(now) is False and sh.loads == 3 and sh.closes == 0
    # FaissQueryable works over it unchanged
    p = pkg.ivf_ann.FaissParams(nprobe=NPROBE)
    pairs = pkg.ivf_ann.FaissQueryable(sh, m).queryWithDistance(q[0], K, p)
    assert [i for i, _ in pairs] == first[0][0].tolist()
    # a newer hour, holding rows near the queries and ids that two older shards hold too: one directory is read, the oldest
    # is closed, the answers change, and the duplicates stay
    write(0, 0, 600)
    assert sh.reload(now) is True
    assert sh.directories == [hour_dir(0), hour_dir(1), hour_dir(2)] and sh.loads == 4 and sh.closes == 1
    second = sh.search(q, K, NPROBE)
    same_answers(second, composed([hour_dir(0), hour_dir(1), hour_dir(2)]))
    assert second[0].tobytes() != first[0].tobytes()
    dup = 0
    for row, cnt in zip(second[0], second[2]):
        got = row[:cnt].tolist()
        dup += len(got) - len(set(got))
    assert dup > 0  # a row of hour 0 and its copy in hour 1 or 2 are both hits
    # two newer hours, the older of them damaged: the reload reads the newest, meets the damaged one and raises; the shard
    # it had read for the new set is closed again, and the index goes on serving the set it had
    write(-1, 600, 900)
    write(-2, 900, 1200)
    with open(os.path.join(hour_dir(-1), "faiss.index"), "r+b") as f:
        f.seek(200)  # inside the centroids
        byte = f.read(1)
        f.seek(200)
        f.write(bytes([byte[0] ^ 0x40]))
    with pytest.raises(ff.FaissFileError, match="CENT.*checksum"):
        sh.reload(now + dt.timedelta(hours=2))
    assert sh.loads == 5 and sh.closes == 2
    assert sh.directories == [hour_dir(0), hour_dir(1), hour_dir(2)]
    same_answers(sh.search(q, K, NPROBE), second)
    # a later reload that finds nothing serves an empty set, as the reference's does once it has started
    assert sh.reload(now + dt.timedelta(hours=500)) is True
    assert sh.directories == [] and sh.closes == 5
    none = sh.search(q, K, NPROBE)
    assert none[2].tolist() == [0] * 5 and none[0].shape == (5, K)
    sh.close()
    assert sh.closes == 5
    # a root without a valid hour
    empty = ff.HourlyShardedIndex(m, D, tmp_path / "nothing", 3, 24)
    with pytest.raises(RuntimeError, match="Failed to find any shards during startup"):
        empty.reload(now)
    late = ff.HourlyShardedIndex(m, D, root, 3, 2)
    with pytest.raises(RuntimeError, match="Failed to find any shards during startup"):
        late.reload(now + dt.timedelta(hours=48))
