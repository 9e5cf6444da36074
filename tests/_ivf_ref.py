"""CPU restatement of the IVF-Flat index (include/ivf_ann.h): numpy, float64 arithmetic on the fp16-rounded inputs -- the
approach of oracle.py's dense scan.  Test infrastructure only; nothing here runs on the device or calls the library."""
import numpy as np

L2, COSINE, INNER_PRODUCT = 0, 1, 2
RTOL, ATOL = 1e-5, 1e-5  # the project's tolerance for this arithmetic (tests/test_dense_gpu.py)


def low_dimensional(rng, n, d, r=3, eps=0.3):
    """Rows whose distances spread instead of concentrating: r latent dimensions under a random linear map plus eps N(0,1)
    per component.  The rows of tests/test_refine_gpu.py and tests/test_annoy_gpu.py."""
    basis = rng.standard_normal((r, d)) / np.sqrt(r)
    return (rng.standard_normal((n, r)) @ basis + eps * rng.standard_normal((n, d))).astype(np.float32)


def prepare(metric, x):
    """What the index stores / a query becomes: Cosine rows L2-normalised (fp32 division by the fp32 norm), then fp16."""
    x = np.atleast_2d(np.asarray(x, np.float32))
    if metric == COSINE:
        norm = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
        norm[~(norm > 0)] = 1.0
        x = x / norm[:, None]
    return x.astype(np.float16).astype(np.float32)


def distances(metric, a, b):
    """[len(a), len(b)] distances of prepared rows a to prepared rows b, float64: L2 = ||a - b||, else 1 - <a, b>."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    dot = a @ b.T
    if metric == L2:
        sq = (a * a).sum(axis=1)[:, None] + (b * b).sum(axis=1)[None, :] - 2.0 * dot
        return np.sqrt(np.maximum(sq, 0.0))
    return 1.0 - dot


def assign(metric, rows, centroids):
    """Nearest centroid of each prepared row (ties: lower cell number) and the whole distance table."""
    dist = distances(metric, rows, centroids)
    return np.argmin(dist, axis=1).astype(np.int32), dist


def probe(metric, queries, centroids, nprobe):
    """The min(nprobe, nlist) nearest cells of each prepared query, nearest first (ties: lower cell), and the distance table."""
    dist = distances(metric, queries, centroids)
    nprobe = min(nprobe, centroids.shape[0])
    cells = np.arange(centroids.shape[0])
    out = np.stack([np.lexsort((cells, dq))[:nprobe] for dq in dist]).astype(np.int32)
    return out, dist


def search_probed(metric, rows, ids, cells, probes, queries, k):
    """Exhaustive top-k of each prepared query over the union of the lists of the cells in its row of `probes`, ascending by
    (distance, id).  Returns per query (ids, distances) of length <= k, plus the (k+1)-th distance (inf if none)."""
    ids = np.asarray(ids, np.int64)
    dist = distances(metric, queries, rows)
    out = []
    for q in range(len(queries)):
        member = np.flatnonzero(np.isin(cells, probes[q]))
        dq = dist[q, member]
        order = np.lexsort((ids[member], dq))
        nxt = dq[order[k]] if len(order) > k else np.inf
        order = order[:k]
        out.append((ids[member][order], dq[order], nxt))
    return out


def clear_positions(r_dist, nxt):
    """Positions of an ascending distance list whose neighbours on both sides (the one past the end included) are more than
    2 tol away: where an answer within tol of the truth must carry the same id."""
    r_dist = np.asarray(r_dist, np.float64)
    ext = np.concatenate([r_dist, [nxt]])
    tol = ATOL + RTOL * np.abs(ext)
    gap = np.diff(ext)
    clear = np.ones(len(r_dist), bool)
    if len(r_dist):
        clear &= gap > 2 * tol[:-1]
        clear[1:] &= gap[:-1] > 2 * tol[1:-1]
    return clear


def objective(metric, rows, centroids):
    """The k-means objective: mean distance of a prepared row to its nearest centroid (L2: ||x - c||; else 1 - <x, c>)."""
    _, dist = assign(metric, rows, centroids)
    return float(dist.min(axis=1).mean())


class IvfRef:
    """load + add + search, as the header states them."""

    def __init__(self, metric, centroids):
        self.metric = metric
        self.centroids = prepare(metric, centroids)
        self.rows = np.zeros((0, self.centroids.shape[1]), np.float32)
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
        self.rows = np.concatenate([self.rows, rows])
        self.ids = np.concatenate([self.ids, new_ids])
        self.cells = np.concatenate([self.cells, cells])

    def list_sizes(self):
        return np.bincount(self.cells, minlength=len(self.centroids)).astype(np.int64)

    def search(self, queries, k, nprobe):
        """-> (ids [nq, k], dist [nq, k], counts [nq], probes [nq, min(nprobe, nlist)])"""
        q = prepare(self.metric, queries)
        probes, _ = probe(self.metric, q, self.centroids, nprobe)
        res = search_probed(self.metric, self.rows, self.ids, self.cells, probes, q, k)
        ids = np.zeros((len(q), k), np.int64)
        dist = np.zeros((len(q), k), np.float64)
        cnt = np.zeros(len(q), np.int32)
        for i, (r_ids, r_dist, _) in enumerate(res):
            cnt[i] = len(r_ids)
            ids[i, :cnt[i]] = r_ids
            dist[i, :cnt[i]] = r_dist
        return ids, dist, cnt, probes
