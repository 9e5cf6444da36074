"""The host-side slicing of an HNSW search (search_prepared in hnsw_ann.hip) at its three edges: more queries than one launch
takes (65,536), more spilled queries than one slice of the second pass takes (256), and a walk that marks as many nodes as its
undo log holds (65,536) or more -- the branch every index from 8M rows up relies on to leave its visited bitmap clean."""
import numpy as np
import pytest

from _hnsw_cases import compare_walk, flat_graph

pytestmark = pytest.mark.gpu


def test_more_queries_than_one_launch(pkg, oracle):
    """65,537 queries: the second launch starts at row 65,536 of the queries, the outputs and the spill flags."""
    m = pkg.dense_ann.DistanceMetric.L2
    rng = np.random.default_rng(65537)
    x = rng.standard_normal((300, 8)).astype(np.float32)
    q = rng.standard_normal((64, 8)).astype(np.float32)
    nq, k, ef = 65537, 3, 8
    ix = pkg.hnsw_ann.Hnsw.build(m, x, max_m=4, ef_construction=20, seed=1)
    try:
        graph, stored = ix.graph(), ix.stored_vectors()
        pq = oracle.dense_prepare(int(m), q)
        want = [oracle.hnsw_search(int(m), stored, graph, pq[i], k, ef) for i in range(64)]
        assert all(len(w[0]) == k for w in want) and len({tuple(w[0]) for w in want}) > 8
        w_ids = np.stack([w[0] for w in want])
        w_dist = np.stack([w[1] for w in want])
        reps = (nq + 63) // 64
        ids, dist, cnt = ix.search(np.tile(q, (reps, 1))[:nq], k, ef)
        assert np.all(cnt == k)
        assert np.array_equal(ids, np.tile(w_ids, (reps, 1))[:nq])
        assert np.array_equal(dist.view(np.int32), np.tile(w_dist, (reps, 1))[:nq].view(np.int32))
        assert ix.last_stats()["distance_evals"] == sum(w[2] for w in want) * (nq // 64) + want[0][2]
    finally:
        ix.close()


def test_more_spilled_queries_than_one_slice(pkg, oracle, monkeypatch):
    """Candidate queues of 40 + 40 entries: every one of 600 queries outgrows its own and runs again, 256 + 256 + 88."""
    m = pkg.dense_ann.DistanceMetric.L2
    rng = np.random.default_rng(600)
    x = rng.standard_normal((4000, 16)).astype(np.float32)
    q = rng.standard_normal((600, 16)).astype(np.float32)
    ix = pkg.hnsw_ann.Hnsw.build(m, x, max_m=16, ef_construction=60, seed=2)
    try:
        graph = ix.graph()
        monkeypatch.setenv("HNSW_DEBUG_CCAP", "40")
        compare_walk(oracle, ix, m, q, 50, 512, graph)
        assert ix.last_stats()["spilled_queries"] == 600
    finally:
        ix.close()


def _first_pass_evals(cap):
    """Distance evaluations of a walk down the chain that gives up when its candidate queue of `cap` entries is full: every
    expansion polls one candidate and admits 64, so after t expansions the queue holds 63 t + 1, and the first expansion that
    would leave more than `cap` is the last; with the entry point's own distance, 1 + 64 t."""
    return 1 + 64 * (cap // 63 + 1)


@pytest.mark.parametrize("blocks", [1024, 1025])
def test_undo_log_at_its_capacity(pkg, oracle, monkeypatch, blocks):
    """A chain of blocks of 64 nodes on a line, block b at coordinate b, every node linked to the 64 nodes of the next block:
    a query beyond the far end walks every block and marks all 64 * blocks nodes -- 65,536, the last walk the log holds, or
    65,600, which wipes the whole bitmap.  A bitmap left dirty changes the answers of the next searches in the same slots.

    The far walk's candidate queue grows by 63 per block, past the first pass's 1024 (LDS) + 8192 entries, so each of those
    queries is walked twice and last_stats counts both: the pass that gave up, and the full walk of 64 * blocks evaluations."""
    m = pkg.dense_ann.DistanceMetric.L2
    n = 64 * blocks
    x = (np.arange(n) // 64).astype(np.float32)[:, None]
    lists = {(0, i): (((i // 64 + 1) % blocks) * 64 + np.arange(64)).tolist() for i in range(n)}
    graph = flat_graph(lists, 0, 0)
    far = np.full((8, 1), 2000.0, np.float32)
    rng = np.random.default_rng(blocks)
    mixed = np.concatenate([[5.0, 600.0, 2000.0], rng.uniform(0.0, 1000.0, 5)]).astype(np.float32)[:, None]
    monkeypatch.setenv("HNSW_DEBUG_VLOG", "1")
    ix = pkg.hnsw_ann.Hnsw.from_graph(m, x, graph, max_m=32)
    try:
        stored = ix.stored_vectors()
        assert np.array_equal(stored, x)
        f_ids, f_dist, f_evals = oracle.hnsw_search(int(m), stored, graph, far[0], 10, 64)
        assert f_evals == n, "the far query evaluates every node"
        assert oracle.hnsw_search(int(m), stored, graph, mixed[0], 10, 64)[2] < 1000, "the near query stops early"

        def far_search():
            ids, dist, cnt = ix.search(far, 10, 64)
            st = ix.last_stats()
            print(f"blocks {blocks}: {st}")
            assert np.all(cnt == len(f_ids)) and np.all(ids == f_ids[None, :])
            assert np.all(dist.view(np.int32) == f_dist.view(np.int32)[None, :])
            assert st["spilled_queries"] == 8
            assert st["distance_evals"] == 8 * (n + _first_pass_evals(1024 + 8192))

        far_search()
        compare_walk(oracle, ix, m, mixed, 10, 64, graph, stored)
        far_search()
    finally:
        ix.close()
