"""CPU restatement of include/polysemous_ann.h: the cost of a codeword numbering in numpy float64, and the Hamming filter
over what an index exports.  Test infrastructure only; nothing here runs on the device or calls the library."""
import numpy as np

KSUB = 256
_POP = np.array([bin(v).count("1") for v in range(256)], np.int64)


def targets_and_weights(codebook):
    """t and w [256, 256] of a subspace's codewords [256, dsub] (the diagonal is meaningless); flat = std(D) == 0."""
    cb = np.asarray(codebook, np.float32).astype(np.float64)
    diff = cb[:, None, :] - cb[None, :, :]
    D = (diff * diff).sum(axis=2)
    off = ~np.eye(KSUB, dtype=bool)
    mean = D[off].mean()
    sd = np.sqrt(((D[off] - mean) ** 2).mean())
    flat = not sd > 0
    t = np.full((KSUB, KSUB), 4.0) if flat else (D - mean) / sd * np.sqrt(2.0) + 4.0
    return t, np.exp(-np.log(2.0) * t), flat


def cost(codebook, perm):
    """sum over i != j of w[i][j] (t[i][j] - popcount(perm[i] ^ perm[j]))^2."""
    t, w, _ = targets_and_weights(codebook)
    p = np.asarray(perm, np.int64)
    h = _POP[p[:, None] ^ p[None, :]].astype(np.float64)
    off = ~np.eye(KSUB, dtype=bool)
    return float((w * (t - h) ** 2)[off].sum())


def hamming(codes, code):
    """Hamming distance of each row of codes uint8 [n, M] to code uint8 [M]."""
    return _POP[np.asarray(codes, np.uint8) ^ np.asarray(code, np.uint8)[None, :]].sum(axis=1)


def filter_answer(all_ids, all_dist, all_cnt, row_of_id, codes, cells, probes, qcodes, ht, k):
    """The filtered answer from an unfiltered one that holds every row of the probed lists (all_ids / all_dist [nq, K],
    ascending by (distance, id), all_cnt [nq]): the candidates whose exported code is at Hamming distance < ht from the
    query code of their (query, cell) pair, the first k.  row_of_id: id -> add-order position.  Returns (ids [nq, k],
    dist [nq, k] float32 -- the unfiltered answer's own bits --, counts [nq], rows that passed over all queries)."""
    nq = len(all_cnt)
    ids = np.zeros((nq, k), np.int64)
    dist = np.zeros((nq, k), np.float32)
    cnt = np.zeros(nq, np.int32)
    passed = 0
    for qi in range(nq):
        m = int(all_cnt[qi])
        rows = np.array([row_of_id[i] for i in all_ids[qi, :m].tolist()], np.int64)
        keep = np.zeros(m, bool)
        for j, c in enumerate(probes[qi].tolist()):
            mine = cells[rows] == c
            if mine.any():
                keep[mine] = hamming(codes[rows[mine]], qcodes[qi, j]) < ht
        passed += int(keep.sum())
        kk = min(k, int(keep.sum()))
        cnt[qi] = kk
        ids[qi, :kk] = all_ids[qi, :m][keep][:kk]
        dist[qi, :kk] = all_dist[qi, :m][keep][:kk]
    return ids, dist, cnt, passed
