"""The HNSW kernels at every row width.  hnsw_ann.hip instantiates its wave-per-item kernels once per CH = dpad / 64 = 1..8; the
other HNSW tests that compare with a CPU restatement stay at d <= 100 (CH 1 and 2).  Here the walk runs at the first and the
last d of every width, and the device build, append, update and the walk over their result at CH 3..8 -- all bit for bit
against oracle/hnsw_oracle.c and tests/hnsw_update_ref.c."""
import numpy as np
import pytest

from _hnsw_cases import assert_same_graph, boundaries, check_update, compare_walk, draw_levels, update_positions

pytestmark = pytest.mark.gpu

WIDTH_EDGES = [1, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 448, 449, 512]


@pytest.mark.parametrize("metric", ["L2", "Cosine", "InnerProduct"])
@pytest.mark.parametrize("d", WIDTH_EDGES)
def test_walk_at_both_ends_of_every_width(pkg, oracle, metric, d):
    """The graph is the oracle's, loaded, so the walk does not depend on the device builder.  stored_vectors() == dense_prepare
    checks hnsw_prep_rows at every d: the padding to dpad and, for Cosine, the norm summed across the lanes."""
    m = getattr(pkg.dense_ann.DistanceMetric, metric)
    rng = np.random.default_rng(7000 + d)
    x = rng.standard_normal((1200, d)).astype(np.float32)
    levels = draw_levels(rng, 1200, 8)
    stored = oracle.dense_prepare(int(m), x)
    graph = oracle.hnsw_build_batched(int(m), stored, levels, 8, 40)
    q = rng.standard_normal((16, d)).astype(np.float32)
    ix = pkg.hnsw_ann.Hnsw.from_graph(m, x, graph, max_m=8)
    try:
        mine = ix.stored_vectors()
        assert np.array_equal(mine.view(np.int32), stored.view(np.int32)), "the stored rows are dense_prepare's, bit for bit"
        for k, ef in ((10, 64), (100, 300)):
            compare_walk(oracle, ix, m, q, k, ef, graph, mine)
    finally:
        ix.close()


# (metric, n, d, max_m, efc, batch): CH = 3 .. 8
WIDE = [("L2", 1200, 192, 8, 40, 128), ("InnerProduct", 1200, 256, 16, 64, 256), ("Cosine", 1200, 257, 6, 32, 256),
        ("InnerProduct", 1000, 384, 8, 40, 128), ("L2", 1000, 448, 4, 32, 64), ("Cosine", 1000, 512, 8, 40, 128)]


@pytest.mark.parametrize("metric,n,d,max_m,efc,batch", WIDE)
def test_build_append_update_and_walk_at_wide_rows(pkg, oracle, metric, n, d, max_m, efc, batch):
    """The oracle states whole builds only, and an append continues the builder's rounds, so the graph of base ++ 300 rows is
    the oracle's when the base ends on a round boundary of the schedule (tests/test_hnsw_append_gpu.py).  n itself is not one
    for any of these cases: the build of n rows is compared on its own, and the append starts from the last boundary <= n."""
    m = getattr(pkg.dense_ann.DistanceMetric, metric)
    Hnsw = pkg.hnsw_ann.Hnsw
    rng = np.random.default_rng(n + d + max_m)
    n0 = max(b for b in boundaries(n, batch) if b <= n)
    n1 = n0 + 300
    x = rng.standard_normal((n + 300, d)).astype(np.float32)
    levels = draw_levels(rng, n, max_m)
    assert levels[:n0].max() >= 1
    stored = oracle.dense_prepare(int(m), x)

    ix = Hnsw.build(m, x[:n], max_m=max_m, ef_construction=efc, levels=levels, gpu=True, batch=batch)
    try:
        assert np.array_equal(ix.stored_vectors(), stored[:n])
        assert_same_graph(ix.graph(), oracle.hnsw_build_batched(int(m), stored[:n], levels, max_m, efc, batch), "build")
    finally:
        ix.close()

    l1 = np.concatenate([levels[:n0], np.zeros(300, np.int32)])
    ix = Hnsw.build(m, x[:n0], max_m=max_m, ef_construction=efc, levels=levels[:n0], gpu=True, batch=batch)
    try:
        ix.append(x[n0:n1], ef_construction=efc, levels=np.zeros(300, np.int32), batch=batch)
        assert ix.n == n1 and np.array_equal(ix.stored_vectors(), stored[:n1])
        g = ix.graph()
        assert_same_graph(g, oracle.hnsw_build_batched(int(m), stored[:n1], l1, max_m, efc, batch), "append")

        pos = update_positions(rng, g, n1, 150)
        assert g[4] in pos and np.isin(pos, g[1][g[0] > 0]).sum() >= 3, "the entry point and rows of the upper levels"
        new = rng.standard_normal((150, d)).astype(np.float32)
        got, after = check_update(ix, m, max_m, efc, pos, new, batch)
        assert np.array_equal(after[pos], oracle.dense_prepare(int(m), new))

        q = rng.standard_normal((16, d)).astype(np.float32)
        compare_walk(oracle, ix, m, q, 10, 50, got, after)
    finally:
        ix.close()
