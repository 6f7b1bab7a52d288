"""numpy restatement of the full-ranking protocol (ops.full_rank_users), in two forms.

Exact: tables of integers in [-128, 128] (optionally times a power of two) with d <= 512 keep every partial sum of
a dot product below 2^23 in magnitude, so fp32 computes it exactly in every summation order: scores are int64 sums,
the order is (score descending, id ascending), excluded items are removed, the tail is filled with -1 / -inf, and the
HIP result has to match bit for bit.

Toleranced: for real-valued tables the fp64 scores s and the standard bound of an fp32 dot product in any order, with
or without FMA, e[j] = gamma * (sum_k |p_k q_k| + |bu| + |bi| + |b0|), gamma = (d + 3) 2^-24 / (1 - (d + 3) 2^-24),
give derived conditions on a returned list (check_toleranced); none of them is a tuned tolerance."""
import numpy as np

MAX_EXACT = 128


def exclusion_sets(exclude, users):
    """list of sets, one per entry of users; exclude: None, a dict of sets, or (indptr, items) arrays"""
    if exclude is None:
        return [set() for _ in users]
    if isinstance(exclude, dict):
        return [set(int(i) for i in exclude.get(int(u), ())) for u in users]
    indptr, items = (np.asarray(x) for x in exclude)
    return [set(int(i) for i in items[indptr[u]:indptr[u + 1]]) for u in users]


def exact_scores(P, Q, users, biases=None, scale=1.0):
    """int64-exact scores as float32 [n, I]: P, Q hold integers * scale; biases (bu, bi, b0) hold integers * scale^2 (any
    value whose sums stay exact), added as (bu + bi) + b0 in float64 (exact there)"""
    Pi = np.rint(np.asarray(P, np.float64) / scale).astype(np.int64)
    Qi = np.rint(np.asarray(Q, np.float64) / scale).astype(np.int64)
    assert np.abs(Pi).max(initial=0) <= MAX_EXACT and np.abs(Qi).max(initial=0) <= MAX_EXACT and P.shape[1] <= 512
    assert np.array_equal(Pi * scale, np.asarray(P, np.float64)) and np.array_equal(Qi * scale, np.asarray(Q, np.float64))
    s = (Pi[np.asarray(users)] @ Qi.T).astype(np.float64) * (scale * scale)
    if biases is not None:
        bu, bi, b0 = (np.asarray(b, np.float64).reshape(-1) for b in biases)
        s = s + ((bu[np.asarray(users)][:, None] + bi[None, :]) + b0[0])
    out = s.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), s), "scores are not exact in fp32: the exact form does not apply"
    return out


def rank_lists(scores, excl, topk):
    """(ids int64 [n, topk], scores float32 [n, topk]) of score rows: (score descending, NaN first, id ascending),
    excluded ids removed, -1 / -inf fill"""
    n, I = scores.shape
    ids = np.full((n, topk), -1, np.int64)
    out = np.full((n, topk), -np.inf, np.float32)
    for b in range(n):
        s = scores[b].astype(np.float64) + 0.0
        key = np.where(np.isnan(s), np.inf, s)
        nan_first = np.isnan(s)
        order = np.lexsort((np.arange(I), -key, ~nan_first))
        keep = [j for j in order.tolist() if j not in excl[b]][:topk]
        ids[b, :len(keep)] = keep
        out[b, :len(keep)] = scores[b, keep]
    return ids, out


def full_rank_exact(P, Q, users, topk, exclude=None, biases=None, scale=1.0):
    topk = min(int(topk), Q.shape[0])
    return rank_lists(exact_scores(P, Q, users, biases, scale), exclusion_sets(exclude, users), topk)


def check_toleranced(P, Q, users, topk, ids, scores, exclude=None, biases=None):
    """assert the derived conditions of the module docstring on a returned (ids, scores)"""
    P64, Q64 = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    d, I = P.shape[1], Q.shape[0]
    topk = min(int(topk), I)
    u = (d + 3) * 2.0 ** -24
    gamma = u / (1.0 - u)
    excl = exclusion_sets(exclude, users)
    assert ids.shape == (len(users), topk) and scores.shape == ids.shape
    for b, usr in enumerate(users):
        s = P64[usr] @ Q64.T
        mag = np.abs(P64[usr])[None, :] @ np.abs(Q64).T
        mag = mag.reshape(-1)
        if biases is not None:
            bu, bi, b0 = (np.asarray(x, np.float64).reshape(-1) for x in biases)
            s = s + ((bu[usr] + bi) + b0[0])
            mag = mag + abs(bu[usr]) + np.abs(bi) + abs(b0[0])
        e = gamma * mag
        eligible = np.array([j for j in range(I) if j not in excl[b]], np.int64)
        want = min(topk, eligible.size)
        row, sc = ids[b], scores[b].astype(np.float64)
        assert np.all(row[want:] == -1) and np.all(np.isneginf(sc[want:])), (b, "fill")
        got = row[:want]
        assert np.all((got >= 0) & (got < I)) and len(set(got.tolist())) == want, (b, "ids distinct and in range")
        assert not (set(got.tolist()) & excl[b]), (b, "excluded id returned")
        assert np.all(np.abs(sc[:want] - s[got]) <= e[got]), (b, "score outside the fp32 bound")
        assert np.all(sc[1:want] <= sc[:want - 1]), (b, "scores rise")
        same = sc[1:want] == sc[:want - 1]
        assert np.all(got[1:][same] > got[:-1][same]), (b, "equal scores not in ascending id")
        if want:
            rest = np.setdiff1d(eligible, got)
            last = got[-1]
            assert np.all(s[rest] <= s[last] + e[rest] + e[last]), (b, "a better item was left out")
