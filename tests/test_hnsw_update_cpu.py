"""Hnsw.update without a GPU: a hand-derived reInsert, the batched restatement of hnsw_index_update (tests/hnsw_update_ref.c) at
batch = 1 against the unbatched reInsert sequence, the JNI glue's checks, and the exported symbol."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _hnsw_update_ref as ref
import _jni
from _jni import ANN


def _line_graph():
    """Six points on a line, x = 0..5, every one at level 0, entry point 0, maxM = 2 (maxM0 = 4):
    0:[1] 1:[0,2] 2:[1,3] 3:[2,4] 4:[3,5] 5:[4]."""
    lists = [[1], [0, 2], [1, 3], [2, 4], [3, 5], [4]]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
    g = (np.zeros(6, np.int32), np.arange(6, dtype=np.int64), off.astype(np.int64), np.array(sum(lists, []), np.int64), 0, 0)
    x = np.zeros((6, 2), np.float32)
    x[:, 0] = np.arange(6)
    return x, g


@pytest.mark.parametrize("batch", [0, 1, 4])
def test_reinsert_known_answer(batch):
    # Move item 5 from x = 5 to x = 1.25 (exact in fp16; L2 distances to it: 0 -> 1.25, 1 -> 0.25, 2 -> 0.75, 3 -> 1.75,
    # 4 -> 2.75), efConstruction = 10.
    # Relink, layer 0: N(5) = [4]; setCand = 5, 4, then N(4) = [3, 5] adds 3: [5, 4, 3].  v = 4: setCopy = [5, 3] at distances
    #   2.75, 1 from 4; both fit the queue (min(10, 2)); 2 <= maxM0, so the list is the max queue's array order: 5 offered first
    #   is the root, 3 (smaller) stays below it -> N(4) = [5, 3].
    # Wire, layer 0 from the entry point 0 (1.25): expands 0 -> 1 (0.25), 1 -> 2 (0.75), 2 -> 3 (1.75, bound 1.75), 3 -> 4 (2.75,
    #   bound 2.75), 4 -> 5 itself (offered to the candidate queue only, :607-609), 5's old list [4] is visited.  Result queue
    #   {0, 1, 2, 3, 4}: 5 > maxM = 2, so the heuristic polls 1 (0.25, kept), 2 (0.75; d(1, 2) = 1 is not < 0.75, kept) and stops
    #   at maxM -> N(5) = [1, 2].
    # Back links (maxM0 = 4 on layer 0): 1: [0, 2] has room -> [0, 2, 5]; 2: [1, 3] -> [1, 3, 5].
    x, g = _line_graph()
    new = np.array([[1.25, 0.0]], np.float32)
    out, stats = ref.update(0, x, g, 2, 10, new, [5], batch)
    assert ref.as_dict(out) == {(0, 0): [1], (0, 1): [0, 2, 5], (0, 2): [1, 3, 5], (0, 3): [2, 4], (0, 4): [5, 3], (0, 5): [1, 2]}
    assert out[4] == 0 and out[5] == 0
    assert stats[1:] == (1, 0, 0, 0)  # one relink, nothing superseded, no addition already present, no list kept


@pytest.mark.parametrize("batch", [0, 1])
def test_reinsert_known_answer_bounded_queue_and_heuristic(batch):
    # Seven points on a line, x = 0, 1, 2, 3, 4, 5, 6.25, level 0 only, entry point 0, maxM = 1 (maxM0 = 2), efConstruction = 3:
    #   0:[1] 1:[0,2] 2:[1,3] 3:[2,4] 4:[3,5] 5:[4,6] 6:[5].  Item 3 moves to x = 5.25.
    # setCand of 3 on layer 0: 3, then 2 and N(2) = [1, 3] (adds 1), then 4 and N(4) = [3, 5] (adds 5): [3, 2, 1, 4, 5] -- 5
    # entries, so each proposal's queue is bounded by efConstruction = 3 and then goes through the heuristic (3 > maxM0).
    # v = 2: offers 3 (3.25), 1 (1), 4 (2) fill the max queue [3, 1, 4]; 5 (3) < 3.25: poll 3 (4 sifts to the root: [4, 1]),
    #   offer 5 -> [5, 1, 4].  Heuristic, ascending: 1 (kept), 4 (d(1, 4) = 3 is not < 2: kept), maxM0 reached -> N(2) = [1, 4].
    # v = 4: offers 3 (1.25), 2 (2), 1 (3) -> [1, 3, 2]; 5 (1) < 3: poll 1 ([2, 3]), offer 5 -> [2, 3, 5].  Ascending: 5 (kept),
    #   3 (d(5, 3) = 0.25 < 1.25: dropped), 2 (d(5, 2) = 3 is not < 2: kept) -> N(4) = [5, 2].
    # Wire from 0 (ef 3; distances to 3: 0 5.25, 1 4.25, 2 3.25, 4 1.25, 5 0.25, 6 1): 0 -> 1, 1 -> 2, 2 -> 4 (result queue full:
    #   0 polled, bound 4.25), 4 -> 5 (1 polled, bound 3.25), 5 -> 6 (2 polled, bound 1.25), 6's list [5] is visited; 3 is
    #   nobody's neighbour any more.  Result {4, 5, 6} > maxM = 1: the heuristic keeps 5 -> N(3) = [5].
    # Back link to 5: [4, 6] is full (maxM0 = 2): re-selection over 4 (1), 6 (1.25), 3 (0.25) ascending: 3 (kept), 4 (d(3, 4) =
    #   1.25 is not < 1: kept) -> N(5) = [3, 4].
    lists = [[1], [0, 2], [1, 3], [2, 4], [3, 5], [4, 6], [5]]
    off = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int64)
    g = (np.zeros(7, np.int32), np.arange(7, dtype=np.int64), off, np.array(sum(lists, []), np.int64), 0, 0)
    x = np.zeros((7, 2), np.float32)
    x[:, 0] = [0, 1, 2, 3, 4, 5, 6.25]
    out, stats = ref.update(0, x, g, 1, 3, np.array([[5.25, 0.0]], np.float32), [3], batch)
    assert ref.as_dict(out) == {(0, 0): [1], (0, 1): [0, 2], (0, 2): [1, 4], (0, 3): [5], (0, 4): [5, 2], (0, 5): [3, 4], (0, 6): [5]}
    assert stats[1:] == (2, 0, 0, 0)


def test_update_of_a_lone_entry_point_keeps_its_list():
    # Two points: the entry point 0 alone on layer 1, both on layer 0.  Updating 0 walks from 0 itself on layer 1, finds nobody
    # but 0, so the heuristic keeps nobody: the list stays (the reference throws at neighbours.get(0), :439) and is counted.
    g = (np.array([0, 0, 1], np.int32), np.array([0, 1, 0], np.int64), np.array([0, 1, 2, 2], np.int64), np.array([1, 0], np.int64), 0, 1)
    x = np.array([[0.0, 0.0], [1.0, 0.0]], np.float32)
    out, stats = ref.update(0, x, g, 2, 10, np.array([[0.5, 0.0]], np.float32), [0], 1)
    assert ref.as_dict(out) == {(0, 0): [1], (0, 1): [0], (1, 0): []}
    assert stats[4] == 1 and stats[3] >= 1  # the list of layer 1 kept; 1 already holds 0


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("max_m", [2, 4])
def test_batched_at_one_equals_the_reinsert_sequence(oracle, metric, max_m):
    rng = np.random.default_rng(100 * metric + max_m)
    n, d = 300, 12
    x = oracle.dense_prepare(metric, rng.standard_normal((n, d)))
    u = 1.0 - rng.random(n)
    levels = np.minimum(60, (-np.log(u) / np.log(max_m)).astype(np.int32)).astype(np.int32)
    g = oracle.hnsw_build(metric, x, levels, max_m, 24)
    pos = rng.permutation(n)[:60].astype(np.int64)
    pos[0] = g[4]  # the entry point too
    new = oracle.dense_prepare(metric, rng.standard_normal((len(pos), d)))
    a, sa = ref.update(metric, x, g, max_m, 24, new, pos, 1)
    b, sb = ref.update(metric, x, g, max_m, 24, new, pos, 0)
    assert ref.as_dict(a) == ref.as_dict(b)
    assert sa[1:] == sb[1:] and sa[2] == 0
    # rounds of several items differ from the sequence, but stay well formed
    c, sc = ref.update(metric, x, g, max_m, 24, new, pos, 16)
    for (level, item), row in ref.as_dict(c).items():
        assert item not in row and len(set(row)) == len(row) and len(row) <= (2 * max_m if level == 0 else max_m)
    assert sc[0] == 4


def test_update_glue_checks_capacities(pkg):
    pkg.load_library()
    e = _jni.Env()
    x = np.zeros((4, 64), np.float32)
    ids = np.arange(4, dtype=np.int64)
    extra = (40, C.c_int64(1))
    # vectors too small for n x d, ids too small or missing, a negative n: refused before the (fake) index is touched
    _, msg, cls = e.call(ANN, "hnswIndexUpdate", None, C.c_int64(1), C.c_int64(5), 64, e.buffer(x), e.buffer(ids), *extra)
    assert msg and "n x d floats" in msg and cls == "java/lang/RuntimeException"
    _, msg, _ = e.call(ANN, "hnswIndexUpdate", None, C.c_int64(1), C.c_int64(4), 64, e.buffer(x), e.buffer(ids[:3]), *extra)
    assert msg and "n longs" in msg
    _, msg, _ = e.call(ANN, "hnswIndexUpdate", None, C.c_int64(1), C.c_int64(4), 64, e.buffer(x), None, *extra)
    assert msg and "n longs" in msg
    _, msg, _ = e.call(ANN, "hnswIndexUpdate", None, C.c_int64(1), C.c_int64(-1), 64, e.buffer(x), e.buffer(ids), *extra)
    assert msg and "n x d floats" in msg
    _, msg, _ = e.call(ANN, "hnswIndexUpdate", None, C.c_int64(1), C.c_int64(4), 64, e.buffer(x, 4 * 64 * 4 - 1), e.buffer(ids), *extra)
    assert msg and "n x d floats" in msg
    # a null index
    _, msg, _ = e.call(ANN, "hnswIndexUpdate", None, C.c_int64(0), C.c_int64(4), 64, e.buffer(x), e.buffer(ids), *extra)
    assert msg and "index" in msg


def _stub_env():
    """A JNI harness whose hnsw_index_info / hnsw_index_update are the stand-ins of tests/jni_update_stub.c."""
    d = tempfile.mkdtemp(prefix="jniupd_")
    out = os.path.join(d, "libjni_update_stub.so")
    subprocess.run(["gcc", "-shared", "-fPIC", "-O1", "-Wall", "-Wextra", "-Werror", "-DSANN_JNI_MINIMAL", "-I", _jni.JNI,
                    os.path.join(_jni.ROOT, "tests", "jni_harness.c"), os.path.join(_jni.ROOT, "tests", "jni_update_stub.c"),
                    os.path.join(_jni.JNI, "ann_jni.c"), "-o", out, "-Wl,-Bsymbolic", "-L", os.path.join(_jni.ROOT, "the-algorithm_amd"),
                    "-lsimclusters_amd", "-Wl,-rpath," + os.path.join(_jni.ROOT, "the-algorithm_amd"), "-Wl,--allow-shlib-undefined"],
                   check=True)
    lib = C.CDLL(out)
    for name, res in (("jh_env", C.c_void_p), ("jh_buffer", C.c_void_p), ("jh_exception", C.c_char_p), ("jh_exception_class", C.c_char_p),
                      ("stub_update_calls", C.c_int64), ("stub_update_n", C.c_int64)):
        getattr(lib, name).restype = res
    lib.jh_buffer.argtypes = [C.c_void_p, C.c_longlong]
    e = _jni.Env.__new__(_jni.Env)
    e.lib, e.env, e.keep = lib, C.c_void_p(lib.jh_env()), []
    return e


def test_update_glue_checks_the_dimension(pkg):
    pkg.load_library()
    e = _stub_env()
    x = np.zeros((4, 64), np.float32)
    ids = np.arange(4, dtype=np.int64)
    # the stand-in index has d = 32: d = 64 is refused by the glue's hnsw_index_info comparison, the library never called
    _, msg, cls = e.call(ANN, "hnswIndexUpdate", None, C.c_int64(1), C.c_int64(4), 64, e.buffer(x), e.buffer(ids), 40, C.c_int64(1))
    assert msg and "dimension" in msg and cls == "java/lang/RuntimeException"
    assert e.lib.stub_update_calls() == 0
    # d = 0 is refused before the index is asked
    _, msg, _ = e.call(ANN, "hnswIndexUpdate", None, C.c_int64(1), C.c_int64(4), 0, e.buffer(x), e.buffer(ids), 40, C.c_int64(1))
    assert msg and "n x d floats" in msg and e.lib.stub_update_calls() == 0
    # the matching d reaches the library with n rows
    _, msg, _ = e.call(ANN, "hnswIndexUpdate", None, C.c_int64(1), C.c_int64(4), 32, e.buffer(x), e.buffer(ids), 40, C.c_int64(1))
    assert msg is None and e.lib.stub_update_calls() == 1 and e.lib.stub_update_n() == 4


def test_update_is_exported(pkg):
    lib = pkg.load_library()
    for sym in ("hnsw_index_update", "hnsw_index_update_stats"):
        assert hasattr(lib, sym), sym
    hnsw_ann = pkg.hnsw_ann
    assert "hnsw_index_update" in hnsw_ann.PROTOS and hasattr(hnsw_ann.Hnsw, "update") and hasattr(hnsw_ann.Hnsw, "update_stats")
