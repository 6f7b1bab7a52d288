"""numpy restatement of the full-ranking protocol on fp64 scores (ops.*_full_rank_users).

Input: a [n, I] score array (row b belongs to users[b]) and an exclusion, None or a dict of sets or (indptr, items)
arrays.  Per row: excluded ids and NaN scores are dropped, the rest is ordered by (score descending compared as float64
with -0.0 folded to +0.0, id ascending) through np.lexsort, the first topk stay and the tail is filled with -1 (score
-inf).  Nothing here is tuned: the HIP result has to match bit for bit."""
import numpy as np


def exclusion_sets(exclude, users):
    """list of sets, one per entry of users; exclude: None, a dict of sets, or (indptr, items) arrays"""
    if exclude is None:
        return [set() for _ in users]
    if isinstance(exclude, dict):
        return [set(int(i) for i in exclude.get(int(u), ())) for u in users]
    indptr, items = (np.asarray(x) for x in exclude)
    return [set(int(i) for i in items[indptr[u]:indptr[u + 1]]) for u in users]


def rank_lists(scores, topk, users=None, exclude=None):
    """(ids int64 [n, topk], scores [n, topk] in the dtype of `scores`) of the score rows"""
    scores = np.asarray(scores)
    n, I = scores.shape
    excl = exclusion_sets(exclude, range(n) if users is None else users)
    ids = np.full((n, topk), -1, np.int64)
    out = np.full((n, topk), -np.inf, scores.dtype)
    for b in range(n):
        s = scores[b].astype(np.float64) + 0.0                  # -0.0 -> +0.0
        ok = ~np.isnan(s)
        if excl[b]:
            gone = np.fromiter((i for i in excl[b] if 0 <= i < I), np.int64)
            ok[gone] = False
        cand = np.nonzero(ok)[0]
        order = cand[np.lexsort((cand, -s[cand]))][:topk]
        ids[b, :order.size] = order
        out[b, :order.size] = (scores[b] + 0.0)[order]
    return ids, out


def user_csr(rows, user_num):
    """(indptr int64 [user_num + 1], items int32) of a dict user -> iterable of items, every row ascending"""
    indptr = np.zeros(user_num + 1, np.int64)
    items = []
    for u in range(user_num):
        row = sorted(int(i) for i in rows.get(u, ()))
        items.extend(row)
        indptr[u + 1] = len(items)
    return indptr, np.asarray(items, np.int32)
