"""The merge kernel's 128-bit in-register wave sort (wave_sort_desc_k128), alone, through sann_debug_wave_sort with a
negative group count: about 600 groups of 64 keys in one call, against numpy.lexsort on (hi, lo).

The network exchanges with DPP moves under bank masks and with the row / half-wave swaps, decides each step with one
128-bit compare and takes "which lane keeps the larger key" from a literal lane mask: the groups below are chosen so that
a wrong mask, a wrong exchange partner or a compare that looks at too few dwords shows as a wrong order."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _groups():
    """-> (hi, lo, names): uint64 [G, 64] each"""
    rng = np.random.default_rng(1313)
    u64 = lambda shape: rng.integers(0, 2 ** 64, size=shape, dtype=np.uint64)
    hi, lo, names = [], [], []

    def add(name, h, l):
        h, l = np.atleast_2d(np.asarray(h, np.uint64)), np.atleast_2d(np.asarray(l, np.uint64))
        hi.append(h), lo.append(l), names.extend([name] * len(h))

    add("random", u64((300, 64)), u64((300, 64)))
    # the cosine regime: whole clusters tie on the score, the id decides
    five = u64((100, 5))
    pick = rng.integers(0, 5, size=(100, 64))
    ids = np.stack([rng.permutation(1 << 20)[:64] for _ in range(100)]).astype(np.uint64)
    add("five scores, distinct ids", np.take_along_axis(five, pick, axis=1), ids << np.uint64(13))
    # distinct hi, tied lo
    add("distinct hi, tied lo", u64((60, 64)) & ~np.uint64(63 << 20) | rng.permuted(np.tile(np.arange(64, dtype=np.uint64), (60, 1)), axis=1) << np.uint64(20),
        np.repeat(u64((60, 1)), 64, axis=1))
    # keys that differ in exactly one of the four dwords (top bit included): the other three are shared by the group
    for word, shift in (("lo", 0), ("lo", 32), ("hi", 0), ("hi", 32)):
        for rep in range(10):
            base_h, base_l = u64(()) , u64(())
            vals = rng.permutation(np.concatenate([rng.integers(0, 2 ** 32, size=62, dtype=np.uint64),
                                                   np.array([0x80000000, 0x7FFFFFFF], np.uint64)]))
            keep = np.uint64(~(0xFFFFFFFF << shift) & 0xFFFFFFFFFFFFFFFF)
            word_vals = (vals << np.uint64(shift))
            if word == "lo":
                add("one dword: lo>>%d" % shift, np.full(64, base_h), (base_l & keep) | word_vals)
            else:
                add("one dword: hi>>%d" % shift, (base_h & keep) | word_vals, np.full(64, base_l))
    srt_h, srt_l = np.sort(u64((20, 64)), axis=1), u64((20, 64))
    add("ascending", srt_h, srt_l)
    add("descending", srt_h[:, ::-1], srt_l)
    add("ascending in lo", np.repeat(u64((10, 1)), 64, axis=1), np.sort(u64((10, 64)), axis=1))
    add("all equal", np.repeat(u64((20, 1)), 64, axis=1), np.repeat(u64((20, 1)), 64, axis=1))
    add("all zero", np.zeros((10, 64), np.uint64), np.zeros((10, 64), np.uint64))
    # 40 real keys over 24 zero paddings, in every order the merge kernel can meet them
    for rep in range(20):
        h, l = u64(64) | np.uint64(2), u64(64)
        pad = np.arange(64) >= 40 if rep == 0 else rng.permutation(64) >= 40
        h[pad], l[pad] = 0, 0
        add("40 real over 24 zero", h, l)
    return np.concatenate(hi), np.concatenate(lo), names


def test_k128_wave_sort_network(pkg):
    lib = pkg.load_library()
    hi, lo, names = _groups()
    G = len(hi)
    assert 550 <= G <= 700
    buf = np.empty((G, 64, 4), np.uint32)
    buf[..., 0], buf[..., 1] = lo & np.uint64(0xFFFFFFFF), lo >> np.uint64(32)
    buf[..., 2], buf[..., 3] = hi & np.uint64(0xFFFFFFFF), hi >> np.uint64(32)
    got = np.ascontiguousarray(buf.copy())
    assert lib.sann_debug_wave_sort(0, -G, got.ctypes.data_as(C.c_void_p)) == 0, lib.sann_last_error()
    g = got.astype(np.uint64)
    got_lo, got_hi = g[..., 0] | g[..., 1] << np.uint64(32), g[..., 2] | g[..., 3] << np.uint64(32)
    for i in range(G):
        order = np.lexsort((lo[i], hi[i]))[::-1]  # descending by (hi, lo); equal keys are identical, their order is moot
        assert np.array_equal(got_hi[i], hi[i][order]) and np.array_equal(got_lo[i], lo[i][order]), (i, names[i])


def test_positive_count_still_sorts_u32(pkg):
    """the sign of the count alone chooses the network: a positive count is the 32-bit sort, untouched"""
    lib = pkg.load_library()
    v = np.random.default_rng(5).integers(0, 2 ** 32, size=(3, 64), dtype=np.uint64).astype(np.uint32)
    got = np.ascontiguousarray(v.copy())
    assert lib.sann_debug_wave_sort(0, 3, got.ctypes.data_as(C.c_void_p)) == 0, lib.sann_last_error()
    assert np.array_equal(got, -np.sort(-v.astype(np.int64), axis=1))
