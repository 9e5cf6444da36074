"""CPU restatement of include/annoy_ann.h: numpy.  The margin in float32 in the header's fixed order, the queue with its
total order, the stop rule, the distinct set, then a float64 re-score (tests/_ivf_ref.py's distances); and an independent
two-means builder with numpy's own generator, for the quality bound.  Test infrastructure only; nothing here runs on the
device or calls the library."""
import heapq

import numpy as np

from _ivf_ref import ATOL, COSINE, L2, RTOL, clear_positions, distances, low_dimensional, prepare  # noqa: F401
from _refine_ref import rerank

SPLIT, LEAF, FALLBACK = 0, 1, 1

# the input of the quality test: measured without a device (see test_annoy_gpu.test_quality), run on one there
QUALITY = dict(n=4000, d=64, nq=64, n_trees=20, k=10, seed=11)
QUALITY_NUMPY_SEEDS = tuple(range(8))


def pad8(x):
    """float32 [m, d] -> [m, ceil(d / 8) * 8], the padding zero."""
    x = np.atleast_2d(np.asarray(x, np.float32))
    s = (x.shape[1] + 7) // 8 * 8
    out = np.zeros((x.shape[0], s), np.float32)
    out[:, :x.shape[1]] = x
    return out


def margins(normals, q, offsets=None):
    """The header's margin, float32 throughout: normals [m, stride] against q [stride] (or [m, stride]).  Pieces of 8; lane
    l of 64 owns pieces l and l + 64 and adds, from 0, product after product (a rounded multiply, then a rounded add); the
    xor tree o = 32..1; then + offset (L2).  Returns float32 [m]."""
    a = np.asarray(normals, np.float32)
    b = np.broadcast_to(np.asarray(q, np.float32), a.shape)
    m, stride = a.shape
    pieces = stride // 8
    npl = 1 if pieces <= 64 else 2
    full = np.zeros((m, npl * 64 * 8), np.float32)
    prod = np.zeros_like(full)
    prod[:, :stride] = a * b  # float32 multiply, rounded once
    prod = prod.reshape(m, npl, 64, 8)
    acc = np.zeros((m, 64), np.float32)
    for j in range(npl):
        for e in range(8):
            acc = acc + prod[:, j, :, e]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    out = acc[:, 0]
    if offsets is not None:
        out = out + np.asarray(offsets, np.float32)
    return out.astype(np.float32)


def forest_arrays(forest):
    """The flat form of a library forest (the_algorithm_amd.annoy_ann.AnnoyForest) as a dict of numpy arrays."""
    i = forest.info()
    return dict(metric=int(i["metric"]), d=i["d"], n=i["n"], leaf_size=i["leaf_size"], nodes=forest.nodes,
                normals=forest.normals, offsets=forest.offsets, roots=forest.roots, items=forest.items)


def split_numbers(nodes):
    """Per node the number of its split in node order (-1 for a leaf)."""
    is_split = nodes[:, 0] == SPLIT
    return np.where(is_split, np.cumsum(is_split) - 1, -1)


def search_k(n_trees, k, nodes_to_explore):
    return n_trees * max(k, k if nodes_to_explore is None else nodes_to_explore // n_trees)


def walk(fa, qprep, budget, all_margins=None):
    """One query's walk over the forest arrays fa.  qprep: the prepared query, float32 [d].  Returns (sorted distinct
    positions, pops, items collected)."""
    nodes, items = fa["nodes"], fa["items"]
    sn = split_numbers(nodes)
    if all_margins is None:
        all_margins = margins(pad8(fa["normals"].astype(np.float32)), pad8(qprep)[0], fa["offsets"] if fa["metric"] == L2 else None)

    def canon(v):
        v = float(v)
        return 0.0 if v == 0.0 else v

    heap = [(-np.inf, -int(r)) for r in fa["roots"]]  # (bound desc, node desc) as a min-heap of the negations
    heapq.heapify(heap)
    got, collected, pops = set(), 0, 0
    while collected < budget and heap:
        nb, nn = heapq.heappop(heap)
        bound, node = -nb, -nn
        pops += 1
        kind, a, b, _ = nodes[node]
        if kind == LEAF:
            got.update(items[a:a + b].tolist())
            collected += int(b)
        else:
            m = float(all_margins[sn[node]])
            right = canon(m if m < bound else bound)
            left = canon(-m if -m < bound else bound)
            heapq.heappush(heap, (-right, -int(b)))
            heapq.heappush(heap, (-left, -int(a)))
    return np.array(sorted(got), np.int64), pops, collected


def walk_all(fa, qprep, budget):
    """walk() for every prepared query: (list of candidate arrays, pops [nq], collected [nq])."""
    normals = pad8(fa["normals"].astype(np.float32))
    off = fa["offsets"] if fa["metric"] == L2 else None
    qp = pad8(qprep)
    out, pops, coll = [], [], []
    for q in range(len(qp)):
        mg = margins(normals, qp[q], off) if len(normals) else np.zeros(0, np.float32)
        c, p, n = walk(fa, qprep[q], budget, mg)
        out.append(c)
        pops.append(p)
        coll.append(n)
    return out, np.array(pops), np.array(coll)


def rescore(metric, rows, ids, cands, queries, k):
    """Each query's candidates sorted by (float64 distance, id, position): per query (ids, distances, positions) of length
    min(k, candidates) and the (k+1)-th distance (inf if none).  rows and queries prepared.  The re-rank's restatement
    (_refine_ref.rerank), every list whole."""
    return rerank(metric, rows, ids, cands, [len(c) for c in cands], queries, k)


def check_answers(res, got_ids, got_dist, got_cnt, k):
    """The project's rule: counts equal, distances within ATOL + RTOL |d| of the float64 ones, ids equal at every clear
    position, 0 / 0 past the count.  Returns (clear positions, positions) for the cap on unclear ones."""
    clear_n = total = 0
    for q, (r_ids, r_dist, _, nxt) in enumerate(res):
        c = len(r_ids)
        assert got_cnt[q] == c, (q, got_cnt[q], c)
        assert np.allclose(got_dist[q, :c], r_dist, rtol=RTOL, atol=ATOL), (q, np.abs(got_dist[q, :c] - r_dist).max())
        clear = clear_positions(r_dist, nxt)
        assert np.array_equal(got_ids[q, :c][clear], r_ids[clear]), q
        assert not got_ids[q, c:].any() and not got_dist[q, c:].any(), q
        clear_n += int(clear.sum())
        total += c
    return clear_n, total


def unclear_share(res):
    """From the restatement alone: the share of answer positions that are not clear."""
    clear_n = sum(int(clear_positions(r[1], r[3]).sum()) for r in res)
    total = sum(len(r[0]) for r in res)
    return 1.0 - clear_n / max(total, 1)


def exhaustive(metric, rows, ids, queries, k):
    """The float64 truth over all rows, in rescore()'s form."""
    return rescore(metric, rows, ids, [np.arange(len(rows))] * len(queries), queries, k)


def recall(got_ids, counts, truth):
    return float(np.mean([len(set(got_ids[q][:counts[q]].tolist()) & set(truth[q][0].tolist())) / len(truth[q][0])
                          for q in range(len(truth))]))


def numpy_forest(metric, rows_prepared, n_trees, leaf_size, seed, steps=200):
    """An independent builder of the same kind of forest: two-means in float64 with numpy's generator, sides by the sign of
    margins() (zero goes left), at most three redraws of an unbalanced split, then the alternating fallback.  Returns the
    flat arrays as forest_arrays() does."""
    rng = np.random.default_rng(seed)
    x32 = pad8(rows_prepared)
    x = np.asarray(rows_prepared, np.float64)
    n, d = x.shape
    leaf = leaf_size or d + 2
    nodes, normals, offsets, roots, items = [], {}, {}, [], []
    for t in range(n_trees):
        perm = np.arange(n)
        roots.append(len(nodes))
        nodes.append(None)
        stack = [(roots[-1], 0, n)]
        while stack:
            v, b, e = stack.pop()
            cnt = e - b
            if cnt <= leaf:
                nodes[v] = (LEAF, t * n + b, cnt, 0)
                continue
            it = perm[b:e]
            side, flags, nrm, off = None, 0, None, 0.0
            for _ in range(4):
                i, j = rng.choice(cnt, 2, replace=False)
                p, q, ic, jc = x[it[i]].copy(), x[it[j]].copy(), 1, 1
                for r in x[it[rng.integers(0, cnt, steps)]]:
                    di, dj = ic * ((p - r) ** 2).sum(), jc * ((q - r) ** 2).sum()
                    if di < dj:
                        p, ic = (p * ic + r) / (ic + 1), ic + 1
                    elif dj < di:
                        q, jc = (q * jc + r) / (jc + 1), jc + 1
                nn = np.linalg.norm(p - q)
                if not nn > 0:
                    continue
                nrm = ((p - q) / nn).astype(np.float16)
                off = np.float32(-(nrm.astype(np.float64) @ ((p + q) / 2))) if metric == L2 else np.float32(0)
                mg = margins(x32[it], pad8(nrm.astype(np.float32))[0], off if metric == L2 else None)
                side = mg > 0
                if max(side.sum(), cnt - side.sum()) <= 0.99 * cnt:
                    break
                side = None
            if side is None:
                flags, nrm, off = FALLBACK, np.zeros(d, np.float16), np.float32(0)
                side = (np.arange(cnt) & 1).astype(bool)
            perm[b:e] = np.concatenate([it[~side], it[side]])
            nl = int((~side).sum())
            left, right = len(nodes), len(nodes) + 1
            nodes += [None, None]
            nodes[v] = (SPLIT, left, right, flags)
            normals[v], offsets[v] = nrm, off
            stack += [(right, b + nl, e), (left, b, b + nl)]
        items.append(perm.copy())
    nodes = np.array(nodes, np.int32)
    order = [v for v in range(len(nodes)) if nodes[v, 0] == SPLIT]
    return dict(metric=metric, d=d, n=n, leaf_size=leaf, nodes=nodes,
                normals=np.array([normals[v] for v in order], np.float16).reshape(len(order), d),
                offsets=np.array([offsets[v] for v in order], np.float32), roots=np.array(roots, np.int32),
                items=np.concatenate(items).astype(np.int32))


def quality_data():
    """(rows, queries) of the quality test: tests/_refine_ref.py's clustered low-dimensional corpus."""
    from _refine_ref import quality_corpus

    p = QUALITY
    return quality_corpus(p["seed"], n=p["n"], d=p["d"], nq=p["nq"])


def cpu_recall(metric, fa, rows_prepared, q_prepared, k, nodes_to_explore=None):
    """recall@k of the restatement's search over forest arrays fa against the exhaustive float64 truth."""
    n_trees = len(fa["roots"])
    ids = np.arange(1, len(rows_prepared) + 1)
    cands, _, _ = walk_all(fa, q_prepared, search_k(n_trees, k, nodes_to_explore))
    res = rescore(metric, rows_prepared, ids, cands, q_prepared, k)
    truth = exhaustive(metric, rows_prepared, ids, q_prepared, k)
    return recall([r[0] for r in res], [len(r[0]) for r in res], truth)
