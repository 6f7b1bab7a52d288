"""numpy restatement of ops.full_rank_positions and utils.metrics.position_kpis.

Positions.  From a score row the full order of tests/full_rank_oracle.py (score descending, a NaN first, -0.0 equal to
+0.0, equal scores by ascending id) over the items outside the user's exclusion row; a target's position is its index in
that list, -1 when it lies outside [0, I) or inside the exclusion row.  Exact form: int64 scores on integer tables
(full_rank_oracle.exact_scores), to be matched bit for bit.  Toleranced form: fp64 scores s and §24's bound e[j] of an
fp32 dot product give  #{j : s_j - e_j > s_t + e_t} <= pos <= #{j != t : s_j + e_j >= s_t - e_t}  over the eligible j.

KPIs.  A request's KPIs at cutoff K are tests/metrics_oracle.py's on the oracle's own full list cut at min(K, eligible)
- where K exceeds the eligible items the implied list is that short - and full_auc is its 'auc' on the whole list
(kpis_from_lists, kpis_from_positions).  closed_form states the same values as formulas of the positions, the way the
kernel computes them; tests/test_oracle_rank_positions.py pins it to metrics_oracle."""
import numpy as np

import full_rank_oracle as FO
import metrics_oracle as MO

LIST_KPIS = ("precision", "recall", "hit", "mrr", "map", "ndcg", "f1", "auc")


def full_lists(scores, excl):
    """per request the ids of ALL eligible items in rank order (int64 arrays of different lengths)"""
    out = []
    for b in range(scores.shape[0]):
        ids, _ = FO.rank_lists(scores[b:b + 1], [excl[b]], scores.shape[1])
        out.append(ids[0][ids[0] >= 0])
    return out


def target_rows(targets, users):
    """list of int64 arrays (row order), one per entry of users; targets: a dict of sets or (indptr, items) arrays"""
    if isinstance(targets, dict):
        return [np.array(sorted(int(i) for i in targets.get(int(u), ())), np.int64) for u in users]
    indptr, items = (np.asarray(x) for x in targets)
    return [items[indptr[u]:indptr[u + 1]].astype(np.int64) for u in users]


def positions(scores, users, targets, exclude=None):
    """-> (out_indptr int64 [n + 1], pos int32 [T], target scores float32 [T], eligible int32 [n], the full lists)"""
    excl = FO.exclusion_sets(exclude, users)
    rows = target_rows(targets, users)
    lists = full_lists(scores, excl)
    I = scores.shape[1]
    out_indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    pos = np.full(out_indptr[-1], -1, np.int32)
    sc = np.full(out_indptr[-1], -np.inf, np.float32)
    for b, row in enumerate(rows):
        where = np.full(I, -1, np.int64)
        where[lists[b]] = np.arange(lists[b].size)
        for r, t in enumerate(row.tolist()):
            if 0 <= t < I and where[t] >= 0:
                pos[out_indptr[b] + r] = where[t]
                sc[out_indptr[b] + r] = scores[b, t] + np.float32(0.0)
    return out_indptr, pos, sc, np.array([l.size for l in lists], np.int32), lists


def positions_exact(P, Q, users, targets, exclude=None, biases=None, scale=1.0):
    return positions(FO.exact_scores(P, Q, users, biases, scale), users, targets, exclude)


def position_bounds(P, Q, users, targets, exclude=None, biases=None):
    """(lo, hi) int64 [T] of the module docstring for real-valued tables; (-1, -1) for a target that is not ranked"""
    P64, Q64 = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    d, I = P.shape[1], Q.shape[0]
    u = (d + 3) * 2.0 ** -24
    gamma = u / (1.0 - u)
    excl = FO.exclusion_sets(exclude, users)
    lo, hi = [], []
    for b, (usr, row) in enumerate(zip(users, target_rows(targets, users))):
        s = P64[usr] @ Q64.T
        mag = (np.abs(P64[usr])[None, :] @ np.abs(Q64).T).reshape(-1)
        if biases is not None:
            bu, bi, b0 = (np.asarray(x, np.float64).reshape(-1) for x in biases)
            s = s + ((bu[usr] + bi) + b0[0])
            mag = mag + abs(bu[usr]) + np.abs(bi) + abs(b0[0])
        e = gamma * mag
        ok = np.ones(I, bool)
        ok[[j for j in excl[b] if 0 <= j < I]] = False
        for t in row.tolist():
            if not (0 <= t < I) or not ok[t]:
                lo.append(-1)
                hi.append(-1)
                continue
            others = ok.copy()
            others[t] = False
            lo.append(int(np.sum(ok & (s - e > s[t] + e[t]))))
            hi.append(int(np.sum(others & (s + e >= s[t] - e[t]))))
    return np.array(lo, np.int64), np.array(hi, np.int64)


def kpis_from_lists(lists, rows, cutoffs, metrics):
    """-> (per_user {name: float64 [nc, n]}, means {name: float64 [nc]}): metrics_oracle.kpis on every request's full
    list cut at min(K, eligible); 'full_auc': its 'auc' on the whole list.  A request needs at least one target."""
    n, nc = len(lists), len(cutoffs)
    per = {m: np.zeros((nc, n)) for m in metrics}
    for b, (full, row) in enumerate(zip(lists, rows)):
        gt = {0: set(row.tolist())}
        for c, K in enumerate(cutoffs):
            ke = min(int(K), full.size)
            for m in metrics:
                name, k = ("auc", full.size) if m == "full_auc" else (m, ke)
                if k == 0:                                  # no list at all: 0 hits of 0 positions
                    per[m][c, b] = np.nan if name in ("precision", "f1", "auc") else 0.0
                    continue
                p, _, _ = MO.kpis(full[None, :k], gt, [0], [k], [name], item_num=1 << 31)
                per[m][c, b] = p[name][0, 0]
    return per, {m: v.mean(axis=1) for m, v in per.items()}


def kpis_from_positions(out_indptr, pos, gt_len, eligible, cutoffs, metrics):
    """The same KPIs from positions alone, through metrics_oracle.kpis as well: the implied list of length min(K,
    eligible) holds target r at index pos[r] and distinct ids that are no target elsewhere."""
    n = len(out_indptr) - 1
    lists, rows = [], []
    for b in range(n):
        p = np.asarray(pos[out_indptr[b]:out_indptr[b + 1]], np.int64)
        L = int(gt_len[b]) if gt_len is not None else p.size
        full = np.arange(int(eligible[b]), dtype=np.int64) + L      # ids L, L + 1, ...: no target
        full[p[p >= 0]] = np.nonzero(p >= 0)[0]                     # target r is id r
        lists.append(full)
        rows.append(np.arange(L, dtype=np.int64))
    return kpis_from_lists(lists, rows, cutoffs, metrics)


def closed_form(p, gt_len, eligible, K, metric):
    """one request's KPI at cutoff K from its positions p (-1: not ranked), as a formula: h = positions < K, r = the rank
    of a hit among the hits, Ke = min(K, eligible)"""
    p = np.sort(np.asarray(p, np.int64)[np.asarray(p) >= 0])
    with np.errstate(invalid="ignore", divide="ignore"):
        if metric == "full_auc":
            T, E = p.size, int(eligible)
            return np.float64(np.sum((E - T) - (p - np.arange(T)))) / np.float64(T * (E - T))
        hits = p[p < K]
        h, ke, r = hits.size, min(int(K), int(eligible)), np.arange(hits.size)
        pre, rec = np.float64(h) / np.float64(ke), np.float64(h) / np.float64(gt_len)
        if metric == "precision":
            return pre
        if metric == "recall":
            return rec
        if metric == "hit":
            return np.float64(h > 0)
        if metric == "mrr":
            return 1.0 / (p[0] + 1.0) if p.size and p[0] < K else np.float64(0.0)
        if metric == "map":
            return np.cumsum((r + 1.0) / (hits + 1.0))[-1] / h if h else np.float64(0.0)
        if metric == "ndcg":
            return np.cumsum(1 / np.log2(hits + 2.0))[-1] / np.cumsum(1 / np.log2(np.arange(2, h + 2)))[-1] if h else np.float64(0.0)
        if metric == "f1":
            return 2 * pre * rec / (pre + rec)
        if metric == "auc":
            return np.float64(np.sum((ke - 1 - hits) - (h - 1 - r))) / np.float64(h * (ke - h))
    raise ValueError(metric)
