"""CPU restatement of the scalar-quantised inverted-file index (include/ivfsq_ann.h): numpy.  The ranges and the codes are
float32 arithmetic, operation for operation as the header states them; the stored rows, the scaled query (rounded through
np.float16), b_q, the index's inner product and the distances are float64.  Test infrastructure only; nothing here runs on
the device or calls the library."""
import numpy as np

from _ivf_ref import ATOL, RTOL, assign, clear_positions, prepare, probe  # noqa: F401

L2, COSINE, INNER_PRODUCT = 0, 1, 2
F32 = np.float32


def ranges(prepared):
    """(vmin, vdiff) of prepared rows: per component the minimum (a zero is +0) and fl32(max - min)."""
    x = np.asarray(prepared, F32)
    vmin = x.min(axis=0) + F32(0)
    vmax = x.max(axis=0) + F32(0)
    return vmin.astype(F32), (vmax - vmin).astype(F32)


def step_of(vdiff):
    return (np.asarray(vdiff, F32) / F32(255)).astype(F32)


def encode(prepared, vmin, vdiff):
    """uint8 codes: clamp(floor(fl32(fl32(x - vmin) / step)), 0, 255); a component with step == 0 has code 0."""
    x, vmin, step = np.asarray(prepared, F32), np.asarray(vmin, F32), step_of(vdiff)
    safe = np.where(step > 0, step, F32(1))
    t = ((x - vmin[None, :]).astype(F32) / safe[None, :]).astype(F32)
    code = np.clip(np.floor(t), 0, 255)
    code[:, step == 0] = 0
    return code.astype(np.uint8)


def xhat(codes, vmin, vdiff):
    """The stored rows, float64: vmin + (code + 0.5) step."""
    return np.asarray(vmin, np.float64)[None, :] + (np.asarray(codes, np.float64) + 0.5) * step_of(vdiff).astype(np.float64)[None, :]


def scaled_queries(prepared_q, vdiff):
    """s = fp16(fl32(q step)), as float64."""
    q = np.asarray(prepared_q, F32)
    return (q * step_of(vdiff)[None, :]).astype(F32).astype(np.float16).astype(np.float64)


def b_q(prepared_q, vmin, vdiff):
    """fl32(sum_i q[i] (vmin[i] + step[i] / 2)), summed in float64."""
    mid = np.asarray(vmin, np.float64) + 0.5 * step_of(vdiff).astype(np.float64)
    return (np.asarray(prepared_q, np.float64) * mid[None, :]).sum(axis=1).astype(F32).astype(np.float64)


def inner_products(prepared_q, codes, vmin, vdiff):
    """P(q, row) [nq, n], float64."""
    return b_q(prepared_q, vmin, vdiff)[:, None] + scaled_queries(prepared_q, vdiff) @ np.asarray(codes, np.float64).T


def distances(metric, prepared_q, codes, vmin, vdiff):
    """[nq, n] distances of the index, float64: L2 sqrt(max(0, |q|^2 - 2 (P - fl32(|xhat|^2) / 2))), else 1 - P."""
    p = inner_products(prepared_q, codes, vmin, vdiff)
    if metric != L2:
        return 1.0 - p
    xs = (xhat(codes, vmin, vdiff) ** 2).sum(axis=1).astype(F32).astype(np.float64)
    qs = (np.asarray(prepared_q, np.float64) ** 2).sum(axis=1).astype(F32).astype(np.float64)
    return np.sqrt(np.maximum(qs[:, None] - 2.0 * (p - 0.5 * xs[None, :]), 0.0))


def search_probed(dist, ids, cells, probes, k):
    """Top-k of each query over the union of the lists of the cells in its row of `probes`, ascending by (distance, id), over
    the given distance matrix [nq, n].  Per query (ids, distances) of length <= k, plus the (k+1)-th distance (inf if none)."""
    ids = np.asarray(ids, np.int64)
    out = []
    for q in range(dist.shape[0]):
        member = np.flatnonzero(np.isin(cells, probes[q]))
        dq = dist[q, member]
        order = np.lexsort((ids[member], dq))
        nxt = dq[order[k]] if len(order) > k else np.inf
        order = order[:k]
        out.append((ids[member][order], dq[order], nxt))
    return out
