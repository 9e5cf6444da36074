"""CPU restatement of the IVF-PQ index (include/ivfpq_ann.h): numpy.  The residuals r = fl32(x - c) and u = fl32(q - c) are
float32 subtractions, as the contract says; everything after them is float64.  Test infrastructure only; nothing here runs
on the device or calls the library."""
import numpy as np

from _ivf_ref import ATOL, COSINE, INNER_PRODUCT, L2, RTOL, assign, prepare, probe  # noqa: F401

KSUB = 256


def fp32_bound(M, dsub):
    """The widening of the tolerance that follows from the fp32 arithmetic, per unit of S: (M + dsub + d + 4) 2^-24."""
    return (M + dsub + M * dsub + 4) * 2.0 ** -24


def tolerance(metric, value, S, M, dsub):
    """Of a search value: L2 in the squared domain (value = S = s, with 2^-22 s more for the fp32 square root); otherwise
    value = 1 - sim and S = the sum of the absolute values of the elementary products."""
    tol = ATOL + RTOL * np.abs(value) + fp32_bound(M, dsub) * S
    if metric == L2:
        tol = tol + 2.0 ** -22 * np.abs(value)
    return tol


def clear_positions(vals, nxt, tol):
    """_ivf_ref.clear_positions with the tolerance of each position given: the positions of an ascending list whose
    neighbours on both sides (the one past the end, nxt, included) are more than twice their tolerance away."""
    vals = np.asarray(vals, np.float64)
    tol = np.asarray(tol, np.float64)
    gap = np.diff(np.concatenate([vals, [nxt]]))
    clear = np.ones(len(vals), bool)
    if len(vals):
        clear &= gap > 2 * tol
        clear[1:] &= gap[:-1] > 2 * tol[1:]
    return clear


def residuals(rows, centroids, cells):
    """fl32(x - centroid[cell]) of prepared rows."""
    return np.asarray(rows, np.float32) - np.asarray(centroids, np.float32)[np.asarray(cells)]


def sub_distances(res, codebooks):
    """[n, M, 256] float64: ||r_m - cb[m][j]||^2."""
    cb = np.asarray(codebooks, np.float64)
    M, _, dsub = cb.shape
    r = np.asarray(res, np.float64).reshape(len(res), M, dsub)
    out = np.empty((len(res), M, KSUB))
    for m in range(M):
        diff = r[:, m, None, :] - cb[m][None, :, :]
        out[:, m, :] = (diff * diff).sum(axis=2)
    return out


def encode(res, codebooks, got=None):
    """codes uint8 [n, M] (ties: lower j), their distances, the distances of the runners-up and, with got given, those of
    the codes in got: [n, M] each, float64.  1024 rows at a time."""
    n, M = len(res), np.asarray(codebooks).shape[0]
    codes = np.zeros((n, M), np.uint8)
    best, second, at_got = np.zeros((n, M)), np.zeros((n, M)), np.zeros((n, M))
    for r0 in range(0, n, 1024):
        dist = sub_distances(res[r0:r0 + 1024], codebooks)
        part = np.partition(dist, 1, axis=2)
        codes[r0:r0 + 1024] = np.argmin(dist, axis=2)
        best[r0:r0 + 1024], second[r0:r0 + 1024] = part[:, :, 0], part[:, :, 1]
        if got is not None:
            at_got[r0:r0 + 1024] = np.take_along_axis(dist, np.asarray(got[r0:r0 + 1024], np.int64)[:, :, None], axis=2)[:, :, 0]
    return codes, best, second, at_got


def quantisation_error(res, codebooks):
    """Per subspace, the mean float64 distance of a residual piece to its nearest codeword: [M]."""
    return encode(res, codebooks)[1].mean(axis=0)


def tables(metric, q, centroid, codebooks):
    """The pair's table [M, 256] and, for InnerProduct / Cosine, that of the absolute products; plus the start value and
    its absolute-product sum.  q and centroid are prepared (fp16-valued) float32 vectors."""
    cb = np.asarray(codebooks, np.float64)
    M, _, dsub = cb.shape
    if metric == L2:
        u = (np.asarray(q, np.float32) - np.asarray(centroid, np.float32)).astype(np.float64).reshape(M, 1, dsub)
        t = ((u - cb) ** 2).sum(axis=2)
        return t, t, 0.0, 0.0
    qd = np.asarray(q, np.float64)
    prod = qd.reshape(M, 1, dsub) * cb
    qc = qd * np.asarray(centroid, np.float64)
    return prod.sum(axis=2), np.abs(prod).sum(axis=2), float(qc.sum()), float(np.abs(qc).sum())


def adc_search(metric, centroids, codebooks, codes, ids, cells, probes, queries, kmax):
    """For each prepared query: the kmax + 1 best of the rows in the lists of its row of `probes`, ascending by (value, id),
    as (ids, values, S).  value is s (the squared distance) for L2 and 1 - sim otherwise; S is what the tolerance scales
    with.  The entry past kmax, if there is one, is the neighbour of the last position."""
    ids = np.asarray(ids, np.int64)
    codes = np.asarray(codes)
    M = codes.shape[1] if codes.ndim == 2 else np.asarray(codebooks).shape[0]
    members_of = {}
    marange = np.arange(M)
    out = []
    for qi in range(len(queries)):
        vals, esses, rids = [], [], []
        for c in probes[qi]:
            c = int(c)
            if c not in members_of:
                members_of[c] = np.flatnonzero(cells == c)
            mem = members_of[c]
            if len(mem) == 0:
                continue
            t, ta, v0, s0 = tables(metric, queries[qi], centroids[c], codebooks)
            cm = codes[mem].astype(np.int64)
            v = v0 + t[marange[None, :], cm].sum(axis=1)
            s = s0 + ta[marange[None, :], cm].sum(axis=1)
            vals.append(v if metric == L2 else 1.0 - v)
            esses.append(s)
            rids.append(ids[mem])
        if not vals:
            out.append((np.zeros(0, np.int64), np.zeros(0), np.zeros(0)))
            continue
        vals, esses, rids = np.concatenate(vals), np.concatenate(esses), np.concatenate(rids)
        order = np.lexsort((rids, vals))[:kmax + 1]
        out.append((rids[order], vals[order], esses[order]))
    return out


class IvfPqRef:
    """load + add + search, as the header states them."""

    def __init__(self, metric, centroids, codebooks):
        self.metric = metric
        self.centroids = prepare(metric, centroids)
        self.codebooks = np.asarray(codebooks, np.float32)
        self.M, _, self.dsub = self.codebooks.shape
        self.codes = np.zeros((0, self.M), np.uint8)
        self.ids = np.zeros(0, np.int64)
        self.cells = np.zeros(0, np.int32)
        self.with_ids = None

    def add(self, x, ids=None):
        if self.with_ids is not None and self.with_ids != (ids is not None):
            raise ValueError("ids on every add or on none")
        self.with_ids = ids is not None
        rows = prepare(self.metric, x)
        new_ids = np.arange(len(self.ids), len(self.ids) + len(rows), dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
        cells, _ = assign(self.metric, rows, self.centroids)
        codes = encode(residuals(rows, self.centroids, cells), self.codebooks)[0]
        self.codes = np.concatenate([self.codes, codes])
        self.ids = np.concatenate([self.ids, new_ids])
        self.cells = np.concatenate([self.cells, cells])

    def search(self, queries, k, nprobe):
        """-> (ids [nq, k], dist [nq, k] float64, counts [nq], probes [nq, min(nprobe, nlist)])"""
        q = prepare(self.metric, queries)
        probes, _ = probe(self.metric, q, self.centroids, nprobe)
        res = adc_search(self.metric, self.centroids, self.codebooks, self.codes, self.ids, self.cells, probes, q, k)
        ids = np.zeros((len(q), k), np.int64)
        dist = np.zeros((len(q), k), np.float64)
        cnt = np.zeros(len(q), np.int32)
        for i, (r_ids, r_val, _) in enumerate(res):
            m = min(k, len(r_ids))
            cnt[i] = m
            ids[i, :m] = r_ids[:m]
            dist[i, :m] = np.sqrt(r_val[:m]) if self.metric == L2 else r_val[:m]
        return ids, dist, cnt, probes
