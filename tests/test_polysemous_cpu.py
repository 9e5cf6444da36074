"""Polysemous codes (include/polysemous_ann.h) without a GPU: the codeword renumbering against the numpy restatement
tests/_polysemous_ref.py, the exported symbols, argument errors that return before any device call, index_factory and the
queryable's refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _polysemous_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
ITERS = 20000  # annealing steps of a test: a few tenths of a second


def test_library_exports_every_declared_symbol(pkg):
    lib = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "polysemous_ann.h")).read()
    declared = set(re.findall(r"^(?:int |const char \*)((?:polysemous|ivfpq|opq)_[a-z_0-9]+)\s*\(", header, re.M))  # the prose names older functions
    assert "polysemous_optimize_codebook" in declared and "ivfpq_search_ht" in declared and "opq_search_ht" in declared
    assert declared == set(pkg.polysemous_ann.PROTOS)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/polysemous_ann.h but not exported"
    # the older headers and bindings declare none of them
    assert not set(pkg.polysemous_ann.PROTOS) & (set(pkg.ivfpq_ann.PROTOS) | set(pkg.opq_ann.PROTOS))


@pytest.mark.parametrize("dsub", [2, 4, 8])
def test_permutation_costs_and_determinism(pkg, dsub):
    ps = pkg.polysemous_ann
    cb = np.random.default_rng(40 + dsub).standard_normal((256, dsub)).astype(np.float32)
    perm, before, after = ps.optimize_codebook(cb, ITERS, 7)
    assert perm.dtype == np.uint8 and sorted(perm.tolist()) == list(range(256)), "a permutation of 0..255"
    again = ps.optimize_codebook(cb, ITERS, 7)
    assert again[0].tobytes() == perm.tobytes() and again[1:] == (before, after), "equal arguments, equal bytes"
    other = ps.optimize_codebook(cb, ITERS, 8)
    assert sorted(other[0].tolist()) == list(range(256)) and other[1] == before  # (another seed may differ in the rest)
    want_before, want_after = ref.cost(cb, np.arange(256)), ref.cost(cb, perm)
    print(f"dsub={dsub}: cost {before:.6f} -> {after:.6f} in {ITERS} steps (numpy {want_before:.6f} -> {want_after:.6f})")
    assert abs(before - want_before) <= 1e-9 * want_before
    assert abs(after - want_after) <= 1e-9 * want_after
    assert after <= before


def test_all_equal_codebook_gives_the_identity(pkg):
    cb = np.full((256, 4), 0.25, np.float32)
    perm, before, after = pkg.polysemous_ann.optimize_codebook(cb, ITERS, 3)
    assert perm.tolist() == list(range(256)) and before == after
    want = ref.cost(cb, np.arange(256))
    assert ref.targets_and_weights(cb)[2] and abs(before - want) <= 1e-9 * want


def test_shuffled_hypercube_corners_get_cheaper(pkg):
    """Codeword j is the corner of {0,1}^8 whose bits are those of shuffle[j]: D is exactly the Hamming distance of the
    unshuffled numbers, and the numbering that undoes the shuffle has the targets' own geometry."""
    shuffle = np.random.default_rng(5).permutation(256)
    cb = ((shuffle[:, None] >> np.arange(8)[None, :]) & 1).astype(np.float32)
    diff = cb[:, None, :] - cb[None, :, :]
    assert np.array_equal((diff * diff).sum(axis=2), ref._POP[shuffle[:, None] ^ shuffle[None, :]])
    perm, before, after = pkg.polysemous_ann.optimize_codebook(cb, 100000, 11)
    print(f"hypercube corners: cost {before:.6f} -> {after:.6f} in 100000 steps; the unshuffled numbering costs "
          f"{ref.cost(cb, shuffle):.6f}")
    assert sorted(perm.tolist()) == list(range(256))
    assert abs(after - ref.cost(cb, perm)) <= 1e-9 * after and abs(before - ref.cost(cb, np.arange(256))) <= 1e-9 * before
    assert after < before


def test_argument_errors(pkg):
    ps = pkg.polysemous_ann
    lib = ps._lib()
    cb = np.zeros((256, 4), np.float32)
    perm = np.zeros(256, np.uint8)
    a, b = C.c_double(), C.c_double()

    def call(dsub, cbp, iters, permp=perm.ctypes.data):
        return lib.polysemous_optimize_codebook(dsub, cbp, iters, 1, permp, C.byref(a), C.byref(b))

    assert call(4, None, 10) == EINVAL and b"null" in lib.polysemous_last_error()
    assert call(4, cb.ctypes.data, 10, None) == EINVAL
    assert call(0, cb.ctypes.data, 10) == EINVAL and b"dsub" in lib.polysemous_last_error()
    assert call(4, cb.ctypes.data, -1) == EINVAL and b"iters" in lib.polysemous_last_error()
    bad = cb.copy()
    bad[3, 1] = np.inf
    assert call(4, bad.ctypes.data, 10) == EINVAL and b"finite" in lib.polysemous_last_error()
    with pytest.raises(ValueError, match="256"):
        ps.optimize_codebook(np.zeros((255, 4), np.float32))
    # the index entry points: what returns before any device call
    x = np.zeros((300, 32), np.float32)
    h = C.c_void_p()
    out = np.zeros(8, np.int64)
    n32, i64 = C.c_int32(), C.c_int64()
    assert lib.ivfpq_index_train_polysemous(0, 0, 32, 4, 8, 300, x.ctypes.data, 1, 1, -1, C.byref(h)) == EINVAL
    assert b"anneal_iters" in lib.ivfpq_last_error()
    assert lib.ivfpq_index_train_polysemous(0, 0, 32, 4, 5, 300, x.ctypes.data, 1, 1, 10, C.byref(h)) == EINVAL
    assert lib.ivfpq_index_train_polysemous(0, 0, 32, 4, 8, 300, None, 1, 1, 10, C.byref(h)) == EINVAL
    assert lib.opq_index_train_polysemous(0, 0, 40, 32, 4, 8, 300, x.ctypes.data, 1, 1, 1, -1, C.byref(h)) == EINVAL
    assert b"anneal_iters" in lib.opq_last_error()
    assert lib.opq_index_train_polysemous(0, 0, 40, 48, 4, 8, 300, x.ctypes.data, 1, 1, 1, 10, C.byref(h)) == EINVAL
    for ht in (0, 5):
        assert lib.ivfpq_search_ht(None, 1, x.ctypes.data, 1, 1, ht, out.ctypes.data, out.ctypes.data, out.ctypes.data) == EINVAL
        assert lib.opq_search_ht(None, 1, x.ctypes.data, 1, 1, ht, out.ctypes.data, out.ctypes.data, out.ctypes.data) == EINVAL
    assert lib.ivfpq_last_query_codes(None, None, None, None) == EINVAL and lib.opq_last_query_codes(None, None, None, None) == EINVAL
    assert lib.ivfpq_last_ht_stats(None, C.byref(i64)) == EINVAL and lib.opq_last_ht_stats(None, C.byref(i64)) == EINVAL
    assert lib.ivfpq_index_is_polysemous(None, C.byref(n32)) == EINVAL and lib.opq_index_is_polysemous(None, C.byref(n32)) == EINVAL


def test_subspace_seed_and_renumber(pkg):
    ps = pkg.polysemous_ann
    assert ps.mix64(0) == 0 and ps.mix64(1) == 0xB456BCFC34C2CB2C
    assert ps.subspace_seed(1, 0) == ps.mix64(1 + 0x9E3779B97F4A7C15) and ps.subspace_seed(1, 0) != ps.subspace_seed(1, 1)
    cb = np.arange(2 * 256 * 3, dtype=np.float32).reshape(2, 256, 3)
    perms = np.stack([np.roll(np.arange(256), 1), np.arange(256)[::-1]]).astype(np.uint8)
    new = ps.renumber(cb, perms)
    assert np.array_equal(new[0, 255], cb[0, 0]) and np.array_equal(new[0, 0], cb[0, 1]) and np.array_equal(new[1, 255], cb[1, 0])


def test_index_factory(pkg):
    ps, m = pkg.polysemous_ann, pkg.dense_ann.DistanceMetric
    cases = {
        "IVF16,PQ8": (None, 16, 8, True), "IVF16,PQ8x8": (None, 16, 8, True), "IVF16,PQ8np": (None, 16, 8, False),
        "IVF16,PQ8x8np": (None, 16, 8, False), "OPQ8,IVF4,PQ8": (64, 4, 8, True), "OPQ8_32,IVF4,PQ8": (32, 4, 8, True),
        "OPQ8_32,IVF4,PQ8x8": (32, 4, 8, True), "OPQ8_32,IVF4,PQ8np": (32, 4, 8, False), "OPQ8,IVF4,PQ8x8np": (64, 4, 8, False),
    }
    for string, (d_out, nlist, M, poly) in cases.items():
        spec = ps.index_factory(64, string, m.Cosine)
        assert (spec.d_out, spec.nlist, spec.M, spec.polysemous, spec.factory_string) == (d_out, nlist, M, poly, string), string
        assert spec.index_class is (ps.PolysemousIvfPq if d_out is None else ps.PolysemousOpqIvfPq)
        assert spec.dimension == 64 and spec.metric == m.Cosine
    for bad in ["IVF16,Flat", "IVF16,PQ8npx8", "IVF16,PQ8 np", "IVF16,PQ8nP", "IVF16,PQ8x4", "PQ8", "OPQ8,PQ8", "IVF16,PQ8,RFlat",
                "OPQ8_32,IVF4,PQ8npnp", "", None, 7]:
        with pytest.raises(ValueError, match="index_factory"):
            ps.index_factory(64, bad, m.L2)
    with pytest.raises(ValueError, match="must agree"):  # the refusals of the older factory are this one's
        ps.index_factory(64, "OPQ4_32,IVF4,PQ8np", m.L2)
    with pytest.raises(ValueError, match="exceeds"):
        ps.index_factory(64, "OPQ8_128,IVF4,PQ8", m.L2)
    # the older factories keep refusing the `np` suffix, as they did
    for old in (pkg.ivfpq_ann.index_factory, pkg.opq_ann.index_factory):
        with pytest.raises(ValueError, match="unsupported factory string"):
            old(64, "IVF16,PQ8np", m.L2)
    with pytest.raises(ValueError, match="unsupported factory string"):
        pkg.opq_ann.index_factory(64, "OPQ8_32,IVF4,PQ8np", m.L2)
    assert pkg.opq_ann.index_factory(64, "OPQ8_32,IVF4,PQ8", m.L2).M == 8 and pkg.ivfpq_ann.index_factory(64, "IVF16,PQ8", m.L2).M == 8


def test_queryable_passes_ht_and_refuses_the_quantizer_fields(pkg):
    ps, iv, m = pkg.polysemous_ann, pkg.ivf_ann, pkg.dense_ann.DistanceMetric

    class Stub:
        def search(self, q, k, nprobe, ht=0):
            self.seen = (k, nprobe, ht)
            return np.array([[5, 9]], np.int64), np.array([[0.25, 1.5]], np.float32), np.array([2], np.int32)

    stub = Stub()
    qa = ps.PolysemousFaissQueryable(stub, m.Cosine)
    got = qa.queryWithDistance(np.zeros(16, np.float32), 2, iv.FaissParams(nprobe=3, ht=20))
    assert stub.seen == (2, 3, 20) and got == [(5, 0.25), (9, 1.0)], "ht goes through; the Cosine translation is the adapter's"
    qa.query(np.zeros(16, np.float32), 2, iv.FaissParams(nprobe=4))
    assert stub.seen == (2, 4, 0), "ht unset: no filter"
    for field in ("quantizerEf", "quantizerKfactorRf", "quantizerNprobe"):
        with pytest.raises(ValueError, match=field):
            qa.queryWithDistance(np.zeros(16, np.float32), 2, iv.FaissParams(nprobe=3, ht=20, **{field: 2}))
    with pytest.raises(ValueError, match="nprobe"):
        qa.queryWithDistance(np.zeros(16, np.float32), 2, iv.FaissParams(ht=20))
    with pytest.raises(ValueError, match="ht"):  # the older queryable keeps refusing ht
        iv.FaissQueryable(stub, m.Cosine).queryWithDistance(np.zeros(16, np.float32), 2, iv.FaissParams(nprobe=3, ht=20))
    with pytest.raises(TypeError):
        ps.adopt(stub)


def test_filter_restatement_by_hand():
    codes = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [255, 255, 0, 0], [3, 0, 0, 1]], np.uint8)
    assert ref.hamming(codes, np.zeros(4, np.uint8)).tolist() == [0, 1, 16, 3]
    cells = np.array([0, 0, 1, 1], np.int32)
    all_ids = np.array([[13, 10, 12, 11]], np.int64)  # ids 10 + row, ascending by distance
    all_dist = np.array([[0.1, 0.2, 0.3, 0.4]], np.float32)
    qcodes = np.zeros((1, 2, 4), np.uint8)
    qcodes[0, 1] = [255, 255, 0, 0]  # the pair of cell 1
    row_of = {10: 0, 11: 1, 12: 2, 13: 3}
    ids, dist, cnt, passed = ref.filter_answer(all_ids, all_dist, np.array([4]), row_of, codes, cells, np.array([[0, 1]]), qcodes, 2, 3)
    assert cnt.tolist() == [3] and ids[0].tolist() == [10, 12, 11] and dist[0].tolist() == all_dist[0, [1, 2, 3]].tolist() and passed == 3
    ids, dist, cnt, passed = ref.filter_answer(all_ids, all_dist, np.array([4]), row_of, codes, cells, np.array([[0, 1]]), qcodes, 1, 3)
    assert cnt.tolist() == [2] and ids[0].tolist() == [10, 12, 0] and passed == 2
