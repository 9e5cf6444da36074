"""CPU restatement of the grouped index (include/grouped_ann.h): numpy, float64 arithmetic on the fp16-prepared inputs,
with the row preparation, the distances and the tolerance of tests/_ivf_ref.py.  Test infrastructure only; nothing here
runs on the device or calls the library."""
import numpy as np

from _ivf_ref import ATOL, COSINE, INNER_PRODUCT, L2, RTOL, clear_positions, distances, prepare  # noqa: F401


class GroupedRef:
    """build + search, as the header states them."""

    def __init__(self, metric, n_groups, vectors, ids, groups):
        self.metric, self.n_groups = metric, n_groups
        self.rows = prepare(metric, vectors) if len(vectors) else np.zeros((0, np.shape(vectors)[-1]), np.float32)
        self.ids = np.arange(len(self.rows), dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
        self.groups = np.asarray(groups, np.int32)
        bad = np.flatnonzero((self.groups < 0) | (self.groups >= n_groups))
        if len(bad):
            raise ValueError(f"row {bad[0]}: group outside [0, {n_groups})")
        self.members = [np.flatnonzero(self.groups == g) for g in range(n_groups)]

    def group_sizes(self):
        return np.array([len(m) for m in self.members], np.int64)

    def search(self, queries, query_groups, k):
        """Per query (ids, distances, the (k+1)-th distance or inf): the k nearest rows of its group ascending by
        (distance, id); nothing for a group outside [0, n_groups) or without rows."""
        q = prepare(self.metric, queries)
        out = []
        for i, g in enumerate(np.asarray(query_groups)):
            member = self.members[g] if 0 <= g < self.n_groups else np.zeros(0, np.int64)
            if len(member) == 0:
                out.append((np.zeros(0, np.int64), np.zeros(0), np.inf))
                continue
            dq = distances(self.metric, q[i:i + 1], self.rows[member])[0]
            order = np.lexsort((self.ids[member], dq))
            nxt = dq[order[k]] if len(order) > k else np.inf
            order = order[:k]
            out.append((self.ids[member][order], dq[order], nxt))
        return out
