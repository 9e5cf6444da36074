"""max_m = 32, the declared limit of hnsw_ann.hip: level-0 lists of 64 neighbours (one per lane of the wave) and upper lists
of 32.  The other HNSW tests stop at max_m = 16, so a list never fills the wave, lane 63 never takes part in a ballot prefix,
a walk never asks wave_distances for a second round of 32 rows and the relink kernel's candidate set stays far below its
capacity.  Everything is bit for bit against oracle/hnsw_oracle.c and tests/hnsw_update_ref.c."""
import numpy as np
import pytest

from _hnsw_cases import assert_same_graph, boundaries, check_update, compare_walk, draw_levels, flat_graph, update_positions

pytestmark = pytest.mark.gpu

N = 4096
SHORT = {11: 0, 12: 1, 13: 33, 14: 63}  # node -> length of its level-0 list; every other list is full


@pytest.fixture(scope="module")
def full_lists():
    """Level 0: 64 distinct neighbours per node, never the node itself (SHORT's nodes excepted).  100 nodes reach level 1 and
    34 of them level 2 -- a list of exactly 32 others of the same level needs at least 33 nodes there.  The entry point is a
    node of level 2.  Whichever node the descent ends on, its level-0 list is full and only that node is marked: the first
    expansion hands the whole wave fresh neighbours, 64 distances in two rounds of 32."""
    rng = np.random.default_rng(32)
    lists = {}
    for i in range(N):
        nb = rng.choice(N - 1, SHORT.get(i, 64), replace=False)
        lists[(0, i)] = (nb + (nb >= i)).tolist()
    upper = rng.permutation(np.setdiff1d(np.arange(N), list(SHORT)))[:100]
    for level, members in ((1, upper), (2, upper[:34])):
        for i in members:
            others = members[members != i]
            lists[(level, int(i))] = rng.permutation(others)[:32].tolist()
    graph = flat_graph(lists, int(upper[0]), 2)
    sizes = np.diff(graph[2])
    assert (sizes[graph[0] == 0] == 64).sum() == N - len(SHORT) and np.all(sizes[graph[0] > 0] == 32)
    assert sorted(sizes[np.isin(graph[1], list(SHORT)) & (graph[0] == 0)].tolist()) == [0, 1, 33, 63]
    return graph


@pytest.mark.parametrize("metric", ["L2", "Cosine", "InnerProduct"])
@pytest.mark.parametrize("d", [64, 512])
def test_walk_over_full_lists(pkg, oracle, full_lists, metric, d):
    m = getattr(pkg.dense_ann.DistanceMetric, metric)
    rng = np.random.default_rng(d)
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((16, d)).astype(np.float32)
    ix = pkg.hnsw_ann.Hnsw.from_graph(m, x, full_lists, max_m=32)
    try:
        stored = ix.stored_vectors()
        for k, ef in ((10, 64), (200, 800)):
            evals = compare_walk(oracle, ix, m, q, k, ef, full_lists, stored)
            assert ix.last_stats()["distance_evals"] == evals
    finally:
        ix.close()


def test_build_append_update_and_walk_at_both_limits(pkg, oracle):
    """max_m = 32 with ef_construction = 256, the builder's largest beam.  The oracle's graph must itself hold full lists, or
    the comparison would not reach the limit.  As in tests/test_hnsw_widths_gpu.py the append starts from the last round
    boundary <= n; its first call ends on the next one."""
    m = pkg.dense_ann.DistanceMetric.L2
    Hnsw = pkg.hnsw_ann.Hnsw
    n, d, max_m, efc, batch = 3000, 64, 32, 256, 256
    rng = np.random.default_rng(1)
    x = rng.standard_normal((n, d)).astype(np.float32)
    levels = draw_levels(rng, n, max_m)
    extra = rng.standard_normal((500, d)).astype(np.float32)

    stored = oracle.dense_prepare(int(m), x)
    want = oracle.hnsw_build_batched(int(m), stored, levels, max_m, efc, batch)
    sizes = np.diff(want[2])
    s0, s_up = sizes[want[0] == 0], sizes[want[0] > 0]
    print(f"oracle graph: {(s0 == 64).sum()} full level-0 lists, {(s_up == 32).sum()} full upper lists, {(s0 > 32).sum()} level-0 lists above 32")
    assert (s0 == 64).sum() >= 1 and (s_up == 32).sum() >= 1 and (s0 > 32).sum() > 500
    ix = Hnsw.build(m, x, max_m=max_m, ef_construction=efc, levels=levels, gpu=True, batch=batch)
    try:
        assert_same_graph(ix.graph(), want, "build")
    finally:
        ix.close()

    bounds = boundaries(n + 500, batch)
    n0 = max(b for b in bounds if b <= n)
    cut = min(b for b in bounds if b > n0)
    n1 = n0 + 500
    assert n0 < cut < n1
    rows = np.concatenate([x[:n0], extra])
    l1 = np.concatenate([levels[:n0], np.zeros(500, np.int32)])
    ix = Hnsw.build(m, rows[:n0], max_m=max_m, ef_construction=efc, levels=levels[:n0], gpu=True, batch=batch)
    try:
        for a, b in ((n0, cut), (cut, n1)):
            ix.append(rows[a:b], ef_construction=efc, levels=np.zeros(b - a, np.int32), batch=batch)
        g = ix.graph()
        assert_same_graph(g, oracle.hnsw_build_batched(int(m), oracle.dense_prepare(int(m), rows), l1, max_m, efc, batch), "append")
        assert np.diff(g[2])[g[0] == 0].max() == 64

        pos = update_positions(rng, g, n1, 150)
        new = rng.standard_normal((150, d)).astype(np.float32)
        got, after = check_update(ix, m, max_m, efc, pos, new, 64)

        q = rng.standard_normal((16, d)).astype(np.float32)
        compare_walk(oracle, ix, m, q, 200, 800, got, after)
    finally:
        ix.close()
