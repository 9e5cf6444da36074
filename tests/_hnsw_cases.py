"""What the HNSW width, max_m and limit tests share: the level draw, the builder's round schedule, and the three comparisons
(walk, graph, update) against the CPU restatements."""
import numpy as np

import _hnsw_update_ref as ref


def draw_levels(rng, n, max_m):
    u = 1.0 - rng.random(n)
    return np.minimum(60, (-np.log(u) / np.log(max_m)).astype(np.int32)).astype(np.int32)


def boundaries(n, batch):
    """Round boundaries of the builder's schedule: b0 = 1, b_{i+1} = b_i + min(batch, max(1, b_i // 8))."""
    out, b = [1], 1
    while b < n:
        b += min(batch, max(1, b // 8))
        out.append(b)
    return out


def flat_graph(lists, entry, max_level):
    """{(level, item): [neighbours]} -> the flat form Hnsw.from_graph and the oracle take, entries sorted by (level, item)."""
    keys = sorted(lists)
    off = np.concatenate([[0], np.cumsum([len(lists[k]) for k in keys])]).astype(np.int64)
    nb = np.concatenate([np.asarray(lists[k], np.int64) for k in keys] + [np.zeros(0, np.int64)])
    return np.array([k[0] for k in keys], np.int32), np.array([k[1] for k in keys], np.int64), off, nb, int(entry), int(max_level)


def compare_walk(oracle, ix, metric, queries, k, ef, graph, stored=None):
    """ix.search against oracle.hnsw_search over `graph` and the index's own stored rows: counts, ids, order, float bits."""
    stored = ix.stored_vectors() if stored is None else stored
    ids, dist, cnt = ix.search(queries, k, ef)
    pq = oracle.dense_prepare(int(metric), queries)
    evals = 0
    for q in range(len(queries)):
        o_items, o_dist, o_evals = oracle.hnsw_search(int(metric), stored, graph, pq[q], k, ef)
        assert cnt[q] == len(o_items), (q, cnt[q], len(o_items))
        assert np.array_equal(ids[q, :cnt[q]], o_items), f"query {q}: neighbours differ"
        assert np.array_equal(dist[q, :cnt[q]].view(np.int32), o_dist.view(np.int32)), f"query {q}: distance bits differ"
        evals += o_evals
    return evals


def assert_same_graph(got, want, what):
    assert got[4] == want[4] and got[5] == want[5], f"{what}: entry point / max level"
    assert ref.as_dict(got) == ref.as_dict(want), f"{what}: the restated graph, entry for entry"


def update_positions(rng, graph, n, nu):
    """nu positions to update: the entry point first, the rest random, a few rows of the upper levels last."""
    special = list(dict.fromkeys([int(graph[4])] + [int(i) for i in np.unique(graph[1][graph[0] > 0])[:8]]))
    rest = [int(i) for i in rng.permutation(n) if int(i) not in set(special)]
    return np.array(special[:1] + rest[:nu - len(special)] + special[1:], np.int64)


def check_update(ix, metric, max_m, efc, pos, new, batch):
    """ix.update(new, pos) against tests/hnsw_update_ref.c: the graph entry for entry and the five counters."""
    before, stored = ix.graph(), ix.stored_vectors()
    ix.update(new, pos, ef_construction=efc, batch=batch)
    after = ix.stored_vectors()
    untouched = np.setdiff1d(np.arange(ix.n), pos)
    assert np.array_equal(after[untouched], stored[untouched])
    want, ws = ref.update(int(metric), stored, before, max_m, efc, after[pos], pos, batch or 4096)
    got = ix.graph()
    assert_same_graph(got, want, "update")
    st = ix.update_stats()
    assert (st["rounds"], st["relinks"], st["relinks_superseded"], st["additions_already_present"], st["lists_kept"]) == ws
    return got, after
