"""hdistance of oracle/hnsw_oracle.c -- the arithmetic every bit-exact HNSW comparison rests on -- against float64 over the same
fp16-rounded values, at the narrowest row, one element past a 64-wide chunk, an odd width of seven chunks and the widest row.

A complete graph on 48 rows (lists of 47, one level) searched with k = ef = 48 returns every distance.  The bound follows the
summation hdistance specifies: eight accumulators of dpad / 64 chunks of 8 terms each, then a tree of three additions, so a
sum passes through m = dpad / 8 + 3 roundings and |s - s64| <= m * 2^-24 * sum|term| * (1 + 2^-20).  For the dot metrics the
products of fp16 values are exact in float; for L2 the bound is on the sum of squares before the root and carries over as
|sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) with a >= b - bound.  One ulp of the result is added for `1 - s` / sqrtf."""
import numpy as np
import pytest

N = 48
METRICS = {"L2": 0, "Cosine": 1, "InnerProduct": 2}


def _complete_graph(n):
    lv = np.zeros(n, np.int32)
    it = np.arange(n, dtype=np.int64)
    off = np.arange(n + 1, dtype=np.int64) * (n - 1)
    nb = np.concatenate([np.delete(np.arange(n, dtype=np.int64), i) for i in range(n)])
    return lv, it, off, nb, 0, 0


@pytest.mark.parametrize("metric", list(METRICS))
@pytest.mark.parametrize("d", [1, 65, 449, 512])
def test_hdistance_is_float64_within_its_summation_bound(oracle, metric, d):
    mt = METRICS[metric]
    rng = np.random.default_rng(1000 * mt + d)
    x = oracle.dense_prepare(mt, rng.standard_normal((N, d)).astype(np.float32))
    q = oracle.dense_prepare(mt, rng.standard_normal((1, d)).astype(np.float32))[0]
    items, dist, evals = oracle.hnsw_search(mt, x, _complete_graph(N), q, N, N)
    assert evals == N and sorted(items.tolist()) == list(range(N)), "k = ef = n on a complete graph returns every row once"

    dpad = (d + 63) // 64 * 64
    m = dpad // 8 + 3
    x64, q64 = x[items].astype(np.float64), q.astype(np.float64)
    terms = (x64 - q64[None, :]) ** 2 if mt == 0 else x64 * q64[None, :]
    s64 = terms.sum(axis=1)
    bound_s = m * 2.0 ** -24 * np.abs(terms).sum(axis=1) * (1 + 2.0 ** -20)
    if mt == 0:
        d64 = np.sqrt(s64)
        bound = bound_s / (np.sqrt(s64) + np.sqrt(np.maximum(s64 - bound_s, 0.0)))
    else:
        d64 = 1.0 - s64
        bound = bound_s
    bound = bound + np.spacing(np.abs(dist)).astype(np.float64)
    err = np.abs(dist.astype(np.float64) - d64)
    print(f"{metric} d={d}: largest error / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound), (metric, d, float(np.max(err / bound)))

    assert np.all(np.diff(dist) >= 0), "ascending in the oracle's own distances"
    gap = d64[None, :] - d64[:, None]  # gap[i, j] = d64[j] - d64[i]; i is returned before j when i < j
    clear = np.abs(gap) > 2.0 * np.maximum(bound[:, None], bound[None, :])
    before = np.arange(N)[:, None] < np.arange(N)[None, :]
    assert np.all(gap[clear & before] > 0), "float64's order wherever float64 separates two rows by more than twice the bound"
    assert (clear & before).sum() > N, "the data separates most pairs"
