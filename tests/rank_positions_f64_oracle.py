"""numpy restatement of full_rank_positions on fp64 scores (ops.*_full_rank_positions), on top of
tests/rank_f64_oracle.py: the FULL list of a score row - rank_lists with topk = I - is the order; a target's position is its
index in that list, -1 when it is absent (outside [0, I), excluded, or a NaN score), and `eligible` is the list's length.
Nothing here is tuned: the HIP result has to match exactly."""
import numpy as np

import rank_f64_oracle as RO


def positions(scores, targets, users=None, exclude=None):
    """scores [n, I] (row b belongs to users[b]); targets: one sequence of item ids per row, in output order.
    -> (out_indptr int64 [n + 1], pos int32 [T], target scores [T] in the dtype of `scores`, eligible int32 [n]); a
    target's score is the row's value at it, -inf when it is outside [0, I) or excluded"""
    scores = np.asarray(scores)
    n, I = scores.shape
    ids, _ = RO.rank_lists(scores, I, users=users, exclude=exclude)
    excl = RO.exclusion_sets(exclude, range(n) if users is None else users)
    out_indptr = np.zeros(n + 1, np.int64)
    out_indptr[1:] = np.cumsum([len(t) for t in targets])
    pos = np.full(out_indptr[-1], -1, np.int32)
    sc = np.full(out_indptr[-1], -np.inf, scores.dtype)
    eligible = np.zeros(n, np.int32)
    for b in range(n):
        order = ids[b][ids[b] >= 0]
        eligible[b] = order.size
        where = np.full(I, -1, np.int64)
        where[order] = np.arange(order.size)
        for r, t in enumerate(targets[b]):
            t = int(t)
            if 0 <= t < I:
                pos[out_indptr[b] + r] = where[t]
                if t not in excl[b]:
                    sc[out_indptr[b] + r] = scores[b, t]
    return out_indptr, pos, sc, eligible


def target_rows(targets, users):
    """the rows of a target CSR (indptr, items) for every entry of users"""
    indptr, items = (np.asarray(x) for x in targets)
    return [items[indptr[u]:indptr[u + 1]].tolist() for u in users]
