"""include/shard_set.h without a device: the header, the Python prototypes and the library's exports agree, and every
refusal that the header promises "before the first device call" comes back on a machine that has no device to call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1


def _lib(pkg):
    return pkg.shard_set._lib()


def test_abi_header_protos_and_exports_agree(pkg):
    lib = _lib(pkg)
    header = open(os.path.join(ROOT, "include", "shard_set.h")).read()
    declared = set(re.findall(r"\b(shardset_[a-z_0-9]+)\s*\(", header))
    assert declared, "no declarations parsed"
    assert declared == set(pkg.shard_set.PROTOS)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/shard_set.h but not exported"
    syms = subprocess.run(["nm", "-D", "--defined-only", pkg.simclusters_ann.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert set(re.findall(r"\b(shardset_[a-z_0-9]+)\b", syms)) == declared
    assert pkg.ShardSet is pkg.shard_set.ShardSet


def test_null_handles_are_refused_with_a_message(pkg):
    lib = _lib(pkg)
    q = np.zeros((1, 32), np.float32)
    dist, ids, cnt = np.zeros((1, 4), np.float32), np.zeros((1, 4), np.int64), np.zeros(1, np.int32)
    n32, i64, f32 = C.c_int32(), C.c_int64(), C.c_float()
    calls = {
        "create": lambda: lib.shardset_create(0, 32, 0, None),
        "set_members": lambda: lib.shardset_set_members(None, 0, None, None),
        "info": lambda: lib.shardset_info(None, C.byref(n32), None, None, None),
        "search": lambda: lib.shardset_search(None, 1, q.ctypes.data, 4, 1, 0, dist.ctypes.data, ids.ctypes.data, cnt.ctypes.data),
        "last_stats": lambda: lib.shardset_last_stats(None, C.byref(i64), None, None, C.byref(f32), None),
    }
    for name, call in calls.items():
        assert call() == EINVAL, name
        assert b"null" in lib.shardset_last_error(), name
    assert lib.shardset_destroy(None) == 0


def test_compose_checks_every_argument_before_the_device(pkg):
    lib = _lib(pkg)
    nq, k_in, k = 3, 4, 5
    ids, dist = np.zeros((2, nq, k_in), np.int64), np.zeros((2, nq, k_in), np.float32)
    cnt = np.full((2, nq), k_in, np.int32)
    o_ids, o_dist, o_cnt = np.zeros((nq, k), np.int64), np.zeros((nq, k), np.float32), np.zeros(nq, np.int32)

    def call(n_shards=2, nq=nq, k_in=k_in, ids=ids.ctypes.data, dist=dist.ctypes.data, cnt=cnt.ctypes.data, k=k, o_ids=o_ids.ctypes.data,
             o_dist=o_dist.ctypes.data, o_cnt=o_cnt.ctypes.data):
        return lib.shardset_compose(0, n_shards, nq, k_in, ids, dist, cnt, k, o_ids, o_dist, o_cnt), lib.shardset_last_error().decode()

    for kw, word in [(dict(n_shards=0), "n_shards"), (dict(n_shards=-1), "n_shards"), (dict(nq=-1), "nq"), (dict(k=0), "k must"),
                     (dict(k=1025), "k must"), (dict(k_in=1025), "k_in"), (dict(k_in=-1), "k_in"), (dict(ids=None), "null"),
                     (dict(dist=None), "null"), (dict(cnt=None), "null"), (dict(o_ids=None), "null"), (dict(o_dist=None), "null"),
                     (dict(o_cnt=None), "null")]:
        rc, msg = call(**kw)
        assert rc == EINVAL and word in msg, (kw, rc, msg)
    for bad in (-1, k_in + 1):
        cnt[1, 2] = bad
        rc, msg = call()
        assert rc == EINVAL and "count" in msg, (bad, rc, msg)
    cnt[1, 2] = k_in
    # nothing to compose is no error and no device work: NULL arrays are fine with nq = 0
    assert call(nq=0, ids=None, dist=None, cnt=None, o_ids=None, o_dist=None, o_cnt=None)[0] == 0
    # the Python mirror raises the module's error with the status and the text
    try:
        pkg.ShardSet.compose([(ids[0], dist[0], cnt[0])], 0)
    except pkg.shard_set.ShardSetError as e:
        assert e.code == EINVAL and "k must" in e.message
    else:
        raise AssertionError("k = 0 was not refused")
