"""sann_batch_run_after: batches kept in flight on two streams.  The fast unit dispatch carries its own events (the
stop event is what a successor waits on and, at profiling level 1, the closing stamp), so every way the chain can be
driven is run here and every pass compared, bit for bit, with a plain sann_batch_run of the same batch."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def same_results(got, want):
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    for q, n in enumerate(want[2]):
        assert np.array_equal(got[0][q, :n], want[0][q, :n])
        assert np.array_equal(got[1][q, :n].view(np.int64), want[1][q, :n].view(np.int64))


def plain_run(qb):
    qb.run()
    qb.finish()
    return qb.results()


@pytest.fixture(scope="module")
def streams():
    hip = C.CDLL("libamdhip64.so")
    out = []
    for _ in range(2):
        h = C.c_void_p()
        assert hip.hipStreamCreateWithFlags(C.byref(h), 1) == 0  # hipStreamNonBlocking
        out.append(h.value)
    yield out
    for st in out:
        assert hip.hipStreamDestroy(C.c_void_p(st)) == 0


@pytest.fixture(scope="module")
def world(pkg):
    """The corpus and queries of test_sann_gpu.py's `small`, an index per partition count, three configurations and
    what a plain run of each returns (computed once, never written to)."""
    co = pkg.corpus.make_corpus(30000, 1500, seed=21, index_cap=400)
    offs, cids, scs = pkg.corpus.make_queries(24, 1500, seed=22, clusters_per_user=50)
    cfgs = [pkg.SimClustersANNConfig(maxNumResults=400, maxTopTweetsPerCluster=300),
            pkg.SimClustersANNConfig(maxNumResults=37, maxTopTweetsPerCluster=120, annAlgorithm=pkg.ScoringAlgorithm.DotProduct),
            pkg.SimClustersANNConfig(maxNumResults=150, maxTopTweetsPerCluster=200,
                                     annAlgorithm=pkg.ScoringAlgorithm.LogCosineSimilarity)]
    w = {"co": co, "q": (offs, cids, scs), "cfgs": cfgs, "index": {}, "want": {}}
    for P in (1, 8, 32):
        w["index"][P] = pkg.ClusterTweetIndex(co.cluster_ids, co.list_offsets, co.tweet_ids, co.scores, n_partitions=P)
    for P in (8, 32):
        w["want"][P] = []
        for cfg in cfgs:
            qb = pkg.QueryBatch(w["index"][P], offs, cids, scs, cfg, now_ms=co.now_ms)
            w["want"][P].append(plain_run(qb))
            qb.close()
    yield w
    for ix in w["index"].values():
        ix.close()


def batch(pkg, world, P, c, cfg=None):
    offs, cids, scs = world["q"]
    return pkg.QueryBatch(world["index"][P], offs, cids, scs, cfg or world["cfgs"][c], now_ms=world["co"].now_ms)


@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("after_merge", [False, True])
@pytest.mark.parametrize("n_batches", [2, 3])
@pytest.mark.parametrize("P", [8, 32])  # desc_query_kernel<4> and <1>
def test_batches_alternate_on_two_streams(pkg, world, streams, P, n_batches, after_merge, level):
    """Nine passes, two in flight, each behind the previous step's batch: every pass equals the plain run, and the
    kernel times count the finished runs."""
    want = world["want"][P]
    qbs = [batch(pkg, world, P, c) for c in range(n_batches)]
    for qb in qbs:
        qb.set_profiling(level)
    finished = [0] * n_batches
    launched = []

    def retire():
        j, st = launched.pop(0)
        qbs[j].finish(st)
        finished[j] += 1
        same_results(qbs[j].results(), want[j])

    prev = None
    for i in range(9):
        j, st = i % n_batches, streams[i & 1]
        qbs[j].run_after(st, None if prev is None else qbs[prev], after_merge=after_merge)
        prev = j
        launched.append((j, st))
        if len(launched) > 1:
            retire()
    retire()
    assert sum(finished) == 9
    for j, qb in enumerate(qbs):
        unit_ms, merge_ms, n = qb.kernel_times()
        if level == 0:
            assert n == 0
            continue
        assert n == finished[j]
        assert unit_ms > 0.0
        if level == 1:
            assert merge_ms == 0.0
        qb.set_profiling(0)
    for qb in qbs:
        qb.close()


@pytest.mark.parametrize("level", [0, 1])
def test_no_predecessor_itself_and_one_that_never_ran(pkg, world, streams, level):
    want = world["want"][32]
    a, never = batch(pkg, world, 32, 0), batch(pkg, world, 32, 1)
    a.set_profiling(level)
    for after in (None, a, a, never):  # (the second `a`: by then the batch has an event of its own run to find)
        a.run_after(streams[0], after, after_merge=False)
        a.finish(streams[0])
        same_results(a.results(), want[0])
    a.run_after(streams[0], a, after_merge=True)
    a.finish(streams[0])
    same_results(a.results(), want[0])
    if level:
        assert a.kernel_times()[2] == 5 and a.kernel_times()[0] > 0.0
    a.close()
    never.close()


@pytest.mark.parametrize("level", [0, 1])
def test_rerun_while_the_successors_wait_is_pending(pkg, world, streams, level):
    """A runs, B is queued behind A's unit kernel, and A is run again on its stream before anything was waited for:
    A's stop event is bound to the new dispatch while B's wait on the old one is still in the queue."""
    want = world["want"][8]
    a, b = batch(pkg, world, 8, 0), batch(pkg, world, 8, 1)
    for qb in (a, b):
        qb.set_profiling(level)
    for _ in range(3):
        a.run_after(streams[0], None, after_merge=False)
        b.run_after(streams[1], a, after_merge=False)
        a.run_after(streams[0], b, after_merge=False)
        a.finish(streams[0])
        b.finish(streams[1])
        same_results(a.results(), want[0])
        same_results(b.results(), want[1])
    a.close()
    b.close()


def test_batch_with_no_queries_in_the_chain(pkg, world, streams):
    co = world["co"]
    want = world["want"][32]
    empty = pkg.QueryBatch(world["index"][32], np.zeros(1, np.int64), np.empty(0, np.int32), np.empty(0), world["cfgs"][0],
                           now_ms=co.now_ms)
    a = batch(pkg, world, 32, 0)
    for level in (0, 1):
        a.set_profiling(level)
        empty.set_profiling(level)
        a.run_after(streams[0], None, after_merge=False)
        empty.run_after(streams[1], a, after_merge=False)
        a.finish(streams[0])
        a.run_after(streams[0], empty, after_merge=False)  # (a predecessor that launched nothing: nothing to wait for)
        empty.finish(streams[1])
        a.finish(streams[0])
        same_results(a.results(), want[0])
        ids, scores, counts, msz = empty.results()
        assert counts.shape == (0,) and ids.shape[0] == 0
        assert empty.kernel_times()[2] == 0
    a.close()
    empty.close()


@pytest.mark.parametrize("level", [0, 1, 2])
def test_general_path_batch_behind_a_fast_one(pkg, world, streams, level, monkeypatch):
    """A batch created under SANN_FORCE_GENERAL=1 (no Variant leaves the fast path: the switch is the environment's,
    read when the batch is prepared) keeps plain recorded events; it chains behind and in front of fast batches."""
    want = world["want"][8]
    fast = batch(pkg, world, 8, 0)
    monkeypatch.setenv("SANN_FORCE_GENERAL", "1")
    general = batch(pkg, world, 8, 1)
    monkeypatch.delenv("SANN_FORCE_GENERAL")
    for qb in (fast, general):
        qb.set_profiling(level)
    for after_merge in (False, True):
        fast.run_after(streams[0], None, after_merge=after_merge)
        general.run_after(streams[1], fast, after_merge=after_merge)
        fast.finish(streams[0])
        same_results(fast.results(), want[0])
        fast.run_after(streams[0], general, after_merge=after_merge)
        general.finish(streams[1])
        same_results(general.results(), want[1])
        fast.finish(streams[0])
        same_results(fast.results(), want[0])
    assert general.unit_waves()[0] == 0, "the general batch ran a fast unit kernel"
    if level:
        assert fast.kernel_times()[2] == 4 and general.kernel_times()[2] == 2
        assert fast.kernel_times()[0] > 0.0 and general.kernel_times()[0] > 0.0
    fast.close()
    general.close()


@pytest.mark.parametrize("level", [0, 1])
def test_chained_batch_whose_units_overflow(pkg, world, streams, level):
    """P = 1 (test_fast_path_falls_back_when_units_do_not_fit): a unit is a whole query, the fast path flags overflow
    and finish() settles it on the general path -- behind a chain as well, and the next chained batch is exact too."""
    cfgs = [pkg.SimClustersANNConfig(maxNumResults=400, maxTopTweetsPerCluster=400),
            pkg.SimClustersANNConfig(maxNumResults=60, maxTopTweetsPerCluster=350, annAlgorithm=pkg.ScoringAlgorithm.DotProduct)]
    qbs = [batch(pkg, world, 1, 0, cfg) for cfg in cfgs]
    want = [plain_run(qb) for qb in qbs]
    assert qbs[0].stats().n_fallback_units > 0
    for qb in qbs:
        qb.set_profiling(level)
    qbs[0].run_after(streams[0], None, after_merge=False)
    qbs[1].run_after(streams[1], qbs[0], after_merge=False)
    qbs[0].finish(streams[0])
    assert qbs[0].stats().n_fallback_units > 0
    same_results(qbs[0].results(), want[0])
    qbs[0].run_after(streams[0], qbs[1], after_merge=False)
    qbs[1].finish(streams[1])
    same_results(qbs[1].results(), want[1])
    qbs[0].finish(streams[0])
    same_results(qbs[0].results(), want[0])
    for qb in qbs:
        qb.close()
