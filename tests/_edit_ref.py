"""numpy restatement of Metric.Edit (the reference's ann/src/main/scala/com/twitter/ann/common/Metric.scala:189-220): the plain
dynamic programme, one (i, j) double loop of vector operations over all pairs of a case at once, with IEEE == on float32.
This is the truth of tests/test_edit_cpu.py and tests/test_edit_gpu.py; nothing of the library is called here.

Cell (i, j) is the distance of the first i elements of a to the first j of b: (0, j) = j, (i, 0) = i (:197-198); equal elements
take the diagonal (:206-207), unequal ones 1 + min(insert (i, j - 1), delete (i - 1, j), replace (i - 1, j - 1)) (:211-215).
"""
import numpy as np

BOUNDARY_LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256)


def csr(strings):
    """(offsets int64 [n + 1], chars float32) of a list of float32 arrays."""
    offsets = np.zeros(len(strings) + 1, np.int64)
    if strings:
        np.cumsum([len(s) for s in strings], out=offsets[1:])
    chars = np.concatenate([np.asarray(s, np.float32) for s in strings]) if strings else np.zeros(0, np.float32)
    return offsets, chars.astype(np.float32)


def _padded(strings):
    lens = np.array([len(s) for s in strings], np.int64)
    out = np.zeros((len(strings), max(int(lens.max(initial=0)), 1)), np.float32)
    for i, s in enumerate(strings):
        out[i, :len(s)] = s
    return out, lens


def pair_distances(a_strings, b_strings) -> np.ndarray:
    """int32 [p]: distance(a[p], b[p])."""
    assert len(a_strings) == len(b_strings)
    p = len(a_strings)
    if p == 0:
        return np.zeros(0, np.int32)
    a, la = _padded(a_strings)
    b, lb = _padded(b_strings)
    return _chunked(a, la, np.arange(p), b, lb, np.arange(p))


def distance_matrix(queries, rows) -> np.ndarray:
    """int32 [nq, n]: distance(queries[q], rows[r]) for every pair."""
    nq, n = len(queries), len(rows)
    if nq == 0 or n == 0:
        return np.zeros((nq, n), np.int32)
    a, la = _padded(queries)
    b, lb = _padded(rows)
    qi, ri = np.repeat(np.arange(nq), n), np.tile(np.arange(n), nq)
    return _chunked(a, la, qi, b, lb, ri).reshape(nq, n)


CHUNK = 1 << 15  # pairs per pass of the double loop: its rows then stay in cache


def _chunked(a, la, ai, b, lb, bi) -> np.ndarray:
    """The pairs (a[ai[p]], b[bi[p]]), CHUNK at a time."""
    out = np.zeros(len(ai), np.int32)
    for c in range(0, len(ai), CHUNK):
        x, y = ai[c:c + CHUNK], bi[c:c + CHUNK]
        out[c:c + CHUNK] = _table(a[x], la[x], b[y], lb[y])
    return out


def _table(a, la, b, lb) -> np.ndarray:
    p, ma, mb = a.shape[0], int(la.max()), int(lb.max())
    dtype = np.uint8 if max(ma, mb) < 255 else np.uint16  # a cell is at most max(i, j); least + 1 must fit too
    ones = dtype(np.iinfo(dtype).max)
    at, bt = np.ascontiguousarray(a.T), np.ascontiguousarray(b.T)  # [i][pair], [j][pair]
    prev = np.empty((mb + 1, p), dtype)                    # row i - 1 of every pair's table, [j][pair]
    prev[:] = np.arange(mb + 1, dtype=dtype)[:, None]      # (0, j) = j
    cur = np.empty_like(prev)
    diagonal = np.empty(p, dtype)
    out = np.zeros(p, np.int32)
    pick = np.arange(p)
    done = la == 0
    out[done] = prev[lb[done], pick[done]]
    for i in range(1, ma + 1):
        equal = bt[:mb] == at[i - 1][None, :]               # IEEE == on float32: NaN != NaN, -0.0 == 0.0
        take = equal.astype(dtype) * ones                  # all bits set where the elements are equal
        keep = ~take
        cur[0] = i                                         # (i, 0) = i
        for j in range(1, mb + 1):
            cell = cur[j]
            np.minimum(cur[j - 1], prev[j], out=cell)      # insert (i, j - 1), delete (i - 1, j)
            np.minimum(cell, prev[j - 1], out=cell)        # replace (i - 1, j - 1)
            cell += 1
            # where(equal, diagonal, 1 + least) as a bit select: a masked copy costs ten times these three passes
            np.bitwise_and(prev[j - 1], take[j - 1], out=diagonal)
            cell &= keep[j - 1]
            cell |= diagonal
        done = la == i
        if done.any():
            out[done] = cur[lb[done], pick[done]]
        prev, cur = cur, prev
    return out


def top_k(dist_row: np.ndarray, ids: np.ndarray, k: int):
    """The k nearest of one query: (distances, ids), ordered by (distance, id, position)."""
    position = np.arange(len(ids))
    order = np.lexsort((position, ids, dist_row))[:k]
    return dist_row[order].astype(np.int32), ids[order].astype(np.int64)


def random_strings(rng, lengths, alphabet):
    alphabet = np.asarray(alphabet, np.float32)
    return [alphabet[rng.integers(0, len(alphabet), int(n))] for n in lengths]


def mutated(rng, s, length, alphabet):
    """A copy of s cut or padded to `length` with 1 to 5 elements replaced: close to s, so small distances occur."""
    alphabet = np.asarray(alphabet, np.float32)
    r = np.resize(s, length).astype(np.float32) if len(s) and length else alphabet[rng.integers(0, len(alphabet), length)]
    for _ in range(int(rng.integers(1, 6))):
        if length:
            r[rng.integers(0, length)] = alphabet[rng.integers(0, len(alphabet))]
    return r


def grid_pairs(rng, lengths, alphabets):
    """For every (la, lb) of lengths^2 and every alphabet: one random pair and one mutated copy."""
    a, b = [], []
    for alphabet in alphabets:
        for la in lengths:
            for lb in lengths:
                s = random_strings(rng, [la], alphabet)[0]
                a += [s, s]
                b += [random_strings(rng, [lb], alphabet)[0], mutated(rng, s, lb, alphabet)]
    return a, b


def kats():
    """(a, b, distance) known answers; strings as float32 code points."""
    def s(text):
        return np.array([ord(c) for c in text], np.float32)
    nan, inf, one = np.float32(np.nan), np.float32(np.inf), np.float32(1.0)
    return [
        (s("kitten"), s("sitting"), 3),
        (s(""), s("abc"), 3),
        (np.array([nan], np.float32), np.array([nan], np.float32), 1),
        (np.array([-0.0], np.float32), np.array([0.0], np.float32), 0),
        (np.array([inf], np.float32), np.array([inf], np.float32), 0),
        (np.array([one], np.float32), np.array([np.nextafter(one, np.float32(2.0))], np.float32), 1),
    ]
