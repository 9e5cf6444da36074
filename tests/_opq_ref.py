"""CPU restatement of the OPQ pre-transform (include/opq_ann.h): numpy, float64.  What lies behind the transform is
tests/_ivfpq_ref.py.  Test infrastructure only; nothing here runs on the device or calls the library."""
import numpy as np

from _ivfpq_ref import COSINE, INNER_PRODUCT, L2  # noqa: F401


def inner_metric(metric):
    """The metric of the IVF-PQ index behind the transform: Cosine rows are normalised in front, then InnerProduct."""
    return INNER_PRODUCT if metric == COSINE else metric


def prepare(metric, x):
    """float64 [n, d_in]: Cosine rows divided by their norm (a zero row stays), the others as they are."""
    x = np.asarray(x, np.float64)
    if metric != COSINE:
        return x
    norm = np.sqrt((x * x).sum(axis=1, keepdims=True))
    norm[norm == 0] = 1.0
    return x / norm


def transform(metric, A, x):
    """(y, S): y = A x^ in float64 [n, d_out] and S = sum_i |A_ji x^_i|, what the fp32 bound of a component scales with."""
    A = np.asarray(A, np.float64)
    xp = prepare(metric, x)
    return xp @ A.T, np.abs(xp) @ np.abs(A).T


def transform_bound(metric, d_in, S, y):
    """Of a component against float64: (d_in + 1) 2^-24 S -- the fp32 FMA chain of d_in terms takes d_in 2^-24 S of it, which
    leaves 2^-24 S for the fp32 division of every x_i of a Cosine row -- and, Cosine, 3 2^-24 |y| more for the fp32 norm
    (the rounding of the square root to fp32 scales the whole row)."""
    bound = (d_in + 1) * 2.0 ** -24 * S
    if metric == COSINE:
        bound = bound + 3 * 2.0 ** -24 * np.abs(y)
    return bound


def correlation(x, y_hat):
    """(C, S): C = X^T Y^ [d_in, d_out] in float64 and S = sum_rows |x_i y^_j|."""
    x, y = np.asarray(x, np.float64), np.asarray(y_hat, np.float64)
    return x.T @ y, np.abs(x).T @ np.abs(y)


def procrustes(C):
    """The orthonormal-rows A [d_out, d_in] maximising tr(A C): (U V^T)^T of the thin SVD; and the maximum, sum sigma."""
    u, s, vt = np.linalg.svd(np.asarray(C, np.float64), full_matrices=False)
    return (u @ vt).T, float(s.sum())


def default_factory_string(n, dimension):
    """faiss_index_bq_dataset.py:178-188 of the reference."""
    M = 48
    d_out = dimension // M * M
    return ("OPQ%d" % M if d_out == dimension else "OPQ%d_%d" % (M, d_out)) + ",IVF%d,PQ%d" % (n // 20, M)


def pq_numpy(y, M, rounds, rng):
    """A plain numpy product quantiser (k-means per subspace, 256 codewords): the decoding of y, float64."""
    y = np.asarray(y, np.float64)
    n, d = y.shape
    dsub = d // M
    out = np.empty_like(y)
    for m in range(M):
        p = y[:, m * dsub:(m + 1) * dsub]
        cb = p[rng.choice(n, 256, replace=False)].copy()
        for _ in range(rounds + 1):
            d2 = (p * p).sum(axis=1)[:, None] - 2.0 * p @ cb.T + (cb * cb).sum(axis=1)[None, :]
            code = d2.argmin(axis=1)
            for j in np.unique(code):
                cb[j] = p[code == j].mean(axis=0)
        d2 = (p * p).sum(axis=1)[:, None] - 2.0 * p @ cb.T + (cb * cb).sum(axis=1)[None, :]
        out[:, m * dsub:(m + 1) * dsub] = cb[d2.argmin(axis=1)]
    return out
