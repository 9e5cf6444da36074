"""bench.py --dump-outputs without a GPU: what dump_outputs writes for a given answer (float64 files, snowflake ids
split into exact 32-bit halves, nothing past a query's count, a seeded row sample under the size limit)."""
import os

import numpy as np

import bench


def _answer(nq, k, seed):
    rng = np.random.default_rng(seed)
    ids = ((rng.integers(1 << 39, 1 << 40, size=(nq, k), dtype=np.int64)) << 22) | rng.integers(0, 1 << 22, size=(nq, k))
    scores = rng.standard_normal((nq, k))
    counts = rng.integers(0, k + 1, size=nq).astype(np.int32)
    counts[0], counts[-1] = 0, k
    map_sizes = (counts + rng.integers(0, 50, size=nq)).astype(np.int32)
    return ids, scores, counts, map_sizes


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_dump_is_float64_and_exact(tmp_path):
    ids, scores, counts, msz = _answer(64, 400, 1)
    bench.dump_outputs(str(tmp_path), ids, scores, counts, msz)
    a = _load(str(tmp_path))
    assert sorted(a) == ["counts", "map_sizes", "query_index", "scores", "tweet_ids_hi32", "tweet_ids_lo32"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert np.array_equal(a["query_index"], np.arange(64))
    got = a["tweet_ids_hi32"].astype(np.int64) * (1 << 32) + a["tweet_ids_lo32"].astype(np.int64)
    for q in range(64):
        c = counts[q]
        assert np.array_equal(got[q, :c], ids[q, :c])
        assert np.array_equal(a["scores"][q, :c].view(np.int64), scores[q, :c].view(np.int64))
        assert not got[q, c:].any() and not a["scores"][q, c:].any()
    assert np.array_equal(a["counts"], counts) and np.array_equal(a["map_sizes"], msz)


def test_dump_samples_rows_under_the_limit(tmp_path):
    ids, scores, counts, msz = _answer(512, 400, 2)
    limit = 1 << 20
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), ids, scores, counts, msz, limit_bytes=limit)
        assert sum(os.path.getsize(os.path.join(str(tmp_path / d), n)) for n in os.listdir(str(tmp_path / d))) <= limit
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    rows = a["query_index"].astype(np.int64)
    assert 0 < len(rows) < 512 and np.all(np.diff(rows) > 0)
    assert all(np.array_equal(a[n], b[n]) for n in a)  # the sample is fixed
    assert np.array_equal(a["counts"], counts[rows]) and np.array_equal(a["tweet_ids_hi32"][:, 0], np.where(counts[rows] > 0, ids[rows, 0] >> 32, 0))
