"""CPU restatement of the re-rank of include/refine_ann.h: numpy, float64 arithmetic on the fp16-rounded inputs, as
tests/_ivf_ref.py restates the flat scan.  Test infrastructure only; nothing here runs on the device or calls the library."""
import numpy as np

from _ivf_ref import ATOL, COSINE, INNER_PRODUCT, L2, RTOL, clear_positions, distances, prepare  # noqa: F401

# the input of the quality test: fixed without a device by tests/test_refine_cpu.py, run on one by tests/test_refine_gpu.py
QUALITY_SEED = 7
QUALITY = dict(n=4000, d=64, M=8, nlist=16, nprobe=16, nq=64, k=10)


def rerank(metric, rows, ids, candidates, counts, queries, k):
    """rows: the stored (prepared) rows [n, d]; ids [n]; candidates [nq, width] add-order positions with counts[q] of them
    valid; queries: prepared [nq, d].  Each query's candidates sorted by (float64 distance, id, position).  Returns per
    query (ids, distances, positions) of length min(k, counts[q]) and the (k+1)-th distance (inf if none)."""
    rows = np.asarray(rows, np.float64)
    ids = np.asarray(ids, np.int64)
    out = []
    for q in range(len(queries)):
        pos = np.asarray(candidates[q][:counts[q]], np.int64)
        if len(pos) == 0:
            out.append((np.zeros(0, np.int64), np.zeros(0), np.zeros(0, np.int64), np.inf))
            continue
        dq = distances(metric, np.asarray(queries[q:q + 1], np.float64), rows[pos])[0]
        order = np.lexsort((pos, ids[pos], dq))
        nxt = dq[order[k]] if len(order) > k else np.inf
        order = order[:k]
        out.append((ids[pos][order], dq[order], pos[order], nxt))
    return out


def recall(got_ids, counts, truth_ids):
    """Mean over the queries of |got[:count] & truth| / len(truth)."""
    return float(np.mean([len(set(got_ids[q, :counts[q]].tolist()) & set(truth_ids[q].tolist())) / len(truth_ids[q])
                          for q in range(len(truth_ids))]))


def exhaustive(metric, rows, ids, queries, k):
    """The float64 truth over all rows: ids [nq, k] ascending by (distance, id)."""
    ids = np.asarray(ids, np.int64)
    dist = distances(metric, queries, rows)
    return np.stack([ids[np.lexsort((ids, dq))[:k]] for dq in dist])


def quality_corpus(seed, n=4000, d=64, nq=64, n_clusters=16, r=3, eps=0.3):
    """The clustered low-dimensional corpus of the quality test: latent cluster centres of dimension r, N(0, 0.5) latent
    spread, a random linear map into R^d, eps N(0,1) noise per component.  Returns (rows, queries)."""
    rng = np.random.default_rng(seed)
    basis = rng.standard_normal((r, d)) / np.sqrt(r)
    centres = 2.0 * rng.standard_normal((n_clusters, r))
    latent = centres[rng.integers(0, n_clusters, n + nq)] + 0.5 * rng.standard_normal((n + nq, r))
    x = (latent @ basis + eps * rng.standard_normal((n + nq, d))).astype(np.float32)
    return x[:n], x[n:]


def numpy_train(metric, x, nlist, M, seed, rounds=6):
    """Centroids [nlist, d] and codebooks [M, 256, d / M] by a plain numpy Lloyd (float64, deterministic): cells by the
    metric's rule over the prepared rows (the means of InnerProduct / Cosine cells scaled to unit length), then one k-means
    per subspace on the residuals by squared L2.  For bases that ivfpq_index_load / opq_index_load take as given."""
    import _ivfpq_ref as pq

    rng = np.random.default_rng(seed)
    rows = prepare(metric, x).astype(np.float64)
    n, d = rows.shape
    cent = rows[rng.choice(n, nlist, replace=False)].copy()
    for _ in range(rounds):
        cells = np.argmin(distances(metric, rows, cent), axis=1)
        for c in range(nlist):
            if np.any(cells == c):
                cent[c] = rows[cells == c].mean(axis=0)
                if metric != L2:
                    cent[c] /= max(np.linalg.norm(cent[c]), 1e-30)
    cent = prepare(L2, cent.astype(np.float32))  # (rounded to fp16 as the index stores them; unit rows stay as they are)
    cells = np.argmin(distances(metric, rows, cent), axis=1)
    res = pq.residuals(rows.astype(np.float32), cent, cells).astype(np.float64)
    dsub = d // M
    cb = np.zeros((M, 256, dsub))
    for m in range(M):
        r = res[:, m * dsub:(m + 1) * dsub]
        cw = r[rng.choice(n, 256, replace=False)].copy()
        for _ in range(rounds):
            code = np.argmin((r * r).sum(axis=1)[:, None] - 2.0 * r @ cw.T + (cw * cw).sum(axis=1)[None, :], axis=1)
            for j in range(256):
                if np.any(code == j):
                    cw[j] = r[code == j].mean(axis=0)
        cb[m] = cw
    return cent.astype(np.float32), cb.astype(np.float32)


def cpu_refined(metric, x, q, cent, cb, k, k_factors, nprobe):
    """The whole pipeline without a device, ids = positions: numpy ADC (_ivfpq_ref.adc_search) for k * max(k_factors)
    candidates, then rerank for every factor.  Returns ({k_factor: ids [nq, k]}, the exhaustive truth [nq, k])."""
    import _ivfpq_ref as pq

    rows, qp = prepare(metric, x), prepare(metric, q)
    centp = prepare(metric, cent)
    cells, _ = pq.assign(metric, rows, centp)
    codes = pq.encode(pq.residuals(rows, centp, cells), cb)[0]
    probes, _ = pq.probe(metric, qp, centp, nprobe)
    ids = np.arange(len(rows), dtype=np.int64)
    width = k * max(k_factors)
    adc = pq.adc_search(metric, centp, cb, codes, ids, cells, probes, qp, width)
    out = {}
    for kf in k_factors:
        cand = np.full((len(qp), k * kf), -1, np.int64)
        cnt = np.zeros(len(qp), np.int64)
        for i, (r_ids, _, _) in enumerate(adc):
            cnt[i] = min(k * kf, len(r_ids))
            cand[i, :cnt[i]] = r_ids[:cnt[i]]
        res = rerank(metric, rows, ids, cand, cnt, qp, k)
        out[kf] = np.stack([np.pad(r[0], (0, k - len(r[0])), constant_values=-1) for r in res])
    return out, exhaustive(metric, rows, ids, qp, k)
