"""Helpers of tests/test_ivf_hnsw_quantizer_gpu.py: the inputs, the CPU oracle's walk over an exported graph, and the
float64 restatements of _ivf_ref / _ivfpq_ref held against an answer, with their tolerances as they are.  Test
infrastructure only."""
import numpy as np

import _ivf_ref as ref
import _ivfpq_ref as pqref

MAX_UNCLEAR = 0.15  # of the positions of a comparison (tests/test_ivfpq_gpu.py)


def graph_metric(metric):
    """The metric of the graph over the centroids: L2 -> L2, InnerProduct and Cosine -> InnerProduct."""
    return ref.L2 if int(metric) == ref.L2 else ref.INNER_PRODUCT


def fp16_rows(rng, n, d, clusters=12):
    """Clustered rows whose every value is a multiple of 1/64 within [-6, 6]: fp16 represents them exactly, so that every
    preparation of an L2 or InnerProduct index is the identity."""
    centres = rng.integers(-192, 193, (clusters, d))
    x = centres[rng.integers(0, clusters, n)] + rng.integers(-96, 97, (n, d))
    x = (x / 64.0).astype(np.float32)
    assert np.array_equal(x.astype(np.float16).astype(np.float32), x)
    return x


def oracle_walk(oracle, metric, centroids, graph, prepared, k, ef):
    """oracle.hnsw_search of every prepared query over the exported graph and centroids: (cells int32 [nq, k] with -1
    beyond the walk's count, counts [nq])."""
    out = np.full((len(prepared), k), -1, np.int32)
    cnt = np.zeros(len(prepared), np.int32)
    for i, q in enumerate(prepared):
        items, _, _ = oracle.hnsw_search(graph_metric(metric), centroids, graph, q, k, ef)
        out[i, :len(items)] = items
        cnt[i] = len(items)
    return out, cnt


def padded(ids, cnt):
    """A search's ids [nq, k] as cells, -1 beyond each count."""
    out = np.asarray(ids).astype(np.int32)
    out[np.arange(out.shape[1])[None, :] >= np.asarray(cnt)[:, None]] = -1
    return out


def found(probes):
    """The probe export without its -1s: one array of cells per query."""
    return [row[row >= 0] for row in np.asarray(probes)]


def rows_probed(index):
    return int(sum(index.list_sizes()[p].sum() for p in found(index.last_probes())))


def check_flat(metric, prepared_rows, ids, cells, probes, prepared_queries, k, got):
    """tests/test_ivf_gpu.py's _check_search with the probes given.  Returns (unclear, total)."""
    got_ids, got_dist, cnt = got
    want = ref.search_probed(int(metric), prepared_rows, ids, cells, found(probes), prepared_queries, k)
    unclear = total = 0
    for q, (r_ids, r_dist, nxt) in enumerate(want):
        m = len(r_ids)
        assert cnt[q] == m, f"query {q}: count {cnt[q]} != {m}"
        np.testing.assert_allclose(got_dist[q, :m], r_dist, rtol=ref.RTOL, atol=ref.ATOL)
        clear = ref.clear_positions(r_dist, nxt)
        assert np.array_equal(got_ids[q, :m][clear], r_ids[clear])
        assert len(set(got_ids[q, :m].tolist())) == m, "no id twice"
        unclear += int((~clear).sum())
        total += m
    return unclear, total


def check_pq(metric, M, dsub, centroids, codebooks, codes, ids, cells, probes, prepared_queries, k, got):
    """tests/test_ivfpq_gpu.py's _compare over _want with the probes given.  Returns (unclear, total)."""
    got_ids, got_dist, cnt = got
    want = pqref.adc_search(int(metric), centroids, codebooks, codes, ids, cells, found(probes), prepared_queries, k)
    unclear = total = 0
    for q, (r_ids, r_val, r_s) in enumerate(want):
        m = min(k, len(r_ids))
        assert cnt[q] == m, f"query {q}: count {cnt[q]} != {m}"
        if m == 0:
            continue
        tol = pqref.tolerance(int(metric), r_val, r_s, M, dsub)
        g = got_dist[q, :m].astype(np.float64)
        g = g * g if int(metric) == pqref.L2 else g
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


def two_rings():
    """A level-0 graph over eight items: two rings of four with no edge between them, the entry point (item 0) in the
    first.  In the form hnsw_ann.Hnsw.graph() returns."""
    lv = np.zeros(8, np.int32)
    it = np.arange(8, dtype=np.int64)
    nb = np.array([[(i + 1) % 4 + 4 * (i // 4), (i + 3) % 4 + 4 * (i // 4)] for i in range(8)], np.int64).reshape(-1)
    off = np.arange(0, 17, 2, dtype=np.int64)
    return lv, it, off, nb, 0, 0
