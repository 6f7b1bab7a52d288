"""A vectorised numpy restatement of daisy/utils/metrics.py and daisy/model/PopRecommender.py (per-list values and means),
the fixtures of the KPI and MostPop tests, and the regimes under which two implementations are compared.

The oracle is pinned to the REAL reference by tests/golden/make_golden_metrics.py (-> tests/golden/kat_metrics.npz), which
asserts `check_regimes(oracle, reference)` before it writes; the device is then held to the same regimes against the
stored reference values.

Regimes (u = 2^-53, m = the number of terms a value sums; every bound is derived, none measured):
  precision, recall, hit, mrr, auc per list; coverage counts   bitwise (each is one correctly rounded fp64 operation on
                                                               integers); the NaN pattern of auc equal
  f1 per list                                                  within 4 u relative (three roundings each side); NaN equal
  popularity per list, integer item_pop                        bitwise (every partial sum is exact)
  map, ndcg, other popularity, diversity per list              |d| <= 4 m u |v|: m = k (map, ndcg, popularity), k (k - 1) / 2
                                                               (diversity) - the same terms in another order, then
                                                               divided as the reference divides
  every mean                                                   |d| <= 4 n u mean|v_i| + the mean of the per-list bounds;
                                                               bitwise for hit (its sum is an exact integer); NaN when a
                                                               list's value is NaN
"""
import numpy as np

U64 = 2.0 ** -53
PER_USER = ("precision", "recall", "hit", "mrr", "map", "ndcg", "f1", "auc", "popularity", "diversity")
BITWISE = ("precision", "recall", "hit", "mrr", "auc")
DEFAULT_KPIS = ["recall", "mrr", "ndcg", "hit", "precision"]            # basic.yaml

# tag -> n lists, K positions, item_num, users, the lengths of the truth rows (cycled over the users), categories,
# cutoffs, the dtype pred is handed over in, integer item_pop or not, repeated / shuffled owners, seed
FIXTURES = {
    "k1":    dict(n=1, K=1, item_num=1, U=1, gt_lens=[1], C=1, cutoffs=[1], dtype="int64", int_pop=True, seed=11),
    "k5":    dict(n=255, K=5, item_num=63, U=40, gt_lens=[1, 2], C=19, cutoffs=[1, 5], dtype="float32", int_pop=True, seed=12),
    "k7":    dict(n=256, K=7, item_num=64, U=300, gt_lens=[1, 2, 64], C=64, cutoffs=[1, 5, 7], dtype="int32", int_pop=True,
                  seed=13),
    "k50":   dict(n=257, K=50, item_num=65, U=100, gt_lens=[1, 2, 64, 65], C=65, cutoffs=[1, 5, 10, 20, 30, 50],
                  dtype="float32", int_pop=False, seed=14),
    "k63":   dict(n=30, K=63, item_num=5000, U=30, gt_lens=[1, 2, 64, 65, 300], C=19, cutoffs=[1, 10, 63], dtype="int64",
                  int_pop=True, seed=15),
    "k64":   dict(n=30, K=64, item_num=5000, U=30, gt_lens=[1, 2, 64, 65, 300], C=1, cutoffs=[5, 64], dtype="int32",
                  int_pop=False, seed=16),
    "k65":   dict(n=30, K=65, item_num=5000, U=30, gt_lens=[1, 2, 64, 65, 300], C=19, cutoffs=[1, 64, 65], dtype="float32",
                  int_pop=True, seed=17),
    "k130":  dict(n=40, K=130, item_num=5000, U=25, gt_lens=[1, 2, 64, 65, 300], C=65, cutoffs=[1, 5, 64, 65, 128, 130],
                  dtype="int64", int_pop=False, seed=18),
    "n1000": dict(n=1000, K=10, item_num=5000, U=400, gt_lens=[1, 2, 64, 65, 300], C=19, cutoffs=[1, 5, 10], dtype="float32",
                  int_pop=False, seed=19, no_diversity=True),
}
# the fixtures whose cutoffs are calc_ranking_results' own for config['topk'] = K
CALC_FIXTURES = ("k7", "k50")
# ('map' has no display name in the reference, 'f1' and 'auc' are out of its dispatch's reach: metrics.py:5-16, :87-90)
CALC_KPIS = ["recall", "mrr", "ndcg", "hit", "precision", "coverage", "popularity", "diversity"]

# MostPop: item_num, interactions (None: item i occurs perm[i] times, perm a permutation of 1..item_num - all counts
# distinct), users, candidates per user, topk, seed
POP_FIXTURES = {
    "distinct": dict(item_num=40, nnz=None, users=25, cands=30, topk=10, seed=31),
    "ties":     dict(item_num=200, nnz=60, users=25, cands=30, topk=10, seed=32),
    "one":      dict(item_num=50, nnz=300, users=9, cands=1, topk=1, seed=33),
    "wide":     dict(item_num=3000, nnz=20000, users=5, cands=1000, topk=10, seed=34),
}


def fixture_metrics(fx):
    return [m for m in PER_USER if not (m == "diversity" and fx.get("no_diversity"))] + ["coverage"]


def make_fixture(tag):
    """-> dict(test_ur {user: set}, test_u list, pred int64 [n, K], item_pop float64 [item_num], i_categories int64
    [item_num, C]) from the fixture's seed.  Owners repeat and are out of order; list 1 has no hit, list 2 only hits (with
    repeats when the row is shorter than K), list 3 repeats a hit id at both ends, ids 0 and item_num - 1 occur."""
    fx = FIXTURES[tag]
    rng = np.random.default_rng(fx["seed"])
    n, K, I, U = fx["n"], fx["K"], fx["item_num"], fx["U"]
    test_ur = {}
    for u in range(U):
        ln = min(fx["gt_lens"][u % len(fx["gt_lens"])], I)
        test_ur[u] = set(int(x) for x in rng.choice(I, ln, replace=False))
    test_u = rng.integers(0, U, n)
    pred = rng.integers(0, I, (n, K))
    for r in range(n):
        T = np.fromiter(test_ur[int(test_u[r])], dtype=np.int64)
        take = rng.random(K) < 0.3
        pred[r, take] = T[rng.integers(0, T.size, int(take.sum()))]
    if n > 1:
        T = test_ur[int(test_u[1])]
        free = np.array([i for i in range(I) if i not in T][:4 * K + 8])
        if free.size:
            pred[1] = free[rng.integers(0, free.size, K)]
    if n > 2:
        T = np.sort(np.fromiter(test_ur[int(test_u[2])], dtype=np.int64))
        pred[2] = T[np.arange(K) % T.size]
    if n > 3 and K > 1:
        t0 = min(test_ur[int(test_u[3])])
        pred[3, 0] = pred[3, K - 1] = t0
    if n > 4:
        pred[4, 0], pred[n - 1, K - 1] = 0, I - 1
    item_pop = rng.integers(0, 1000, I).astype(np.float64)
    if not fx["int_pop"]:
        item_pop = item_pop + rng.random(I)
    cats = (rng.random((I, fx["C"])) < 0.3).astype(np.int64)
    return dict(test_ur=test_ur, test_u=[int(u) for u in test_u], pred=pred.astype(np.int64), item_pop=item_pop,
                i_categories=cats)


def make_pop_fixture(tag):
    """-> dict(items int64 [nnz] (the training item column), us int64 [users], cands int64 [users, cands] distinct per row)"""
    fx = POP_FIXTURES[tag]
    rng = np.random.default_rng(fx["seed"])
    I = fx["item_num"]
    if fx["nnz"] is None:
        items = np.repeat(np.arange(I), rng.permutation(I) + 1)
        rng.shuffle(items)
    else:
        items = rng.integers(0, max(I // 4, 1), fx["nnz"]) if tag == "ties" else rng.integers(0, I, fx["nnz"])
    cands = np.stack([rng.choice(I, fx["cands"], replace=False) for _ in range(fx["users"])])
    return dict(items=items.astype(np.int64), us=np.arange(fx["users"], dtype=np.int64), cands=cands.astype(np.int64))


# ---- MostPop ---------------------------------------------------------------------------------------------------------
def pop_fit(items, item_num):
    cnt = np.bincount(items, minlength=item_num).astype(np.float64)
    return cnt, cnt / (1 + cnt)


def pop_rank(score, cands, topk):
    """score descending, ties to the lower candidate position"""
    order = np.argsort(-score[cands], axis=1, kind="stable")[:, :topk]
    return np.take_along_axis(cands, order, 1)


# ---- the KPIs --------------------------------------------------------------------------------------------------------
def hit_matrix(pred, test_ur, test_u, item_num):
    """r [n, K] bool (np.in1d per list) and the lengths of the truth rows [n]"""
    users = np.asarray(test_u, dtype=np.int64)
    keys = np.array(sorted(u * item_num + i for u in set(users.tolist()) for i in test_ur[u]), dtype=np.int64)
    r = np.isin(users[:, None] * item_num + pred, keys)
    return r, np.array([len(test_ur[u]) for u in users.tolist()], dtype=np.float64)


def first_occurrence(pred):
    """[n, K] bool: no earlier position of the list holds the same id"""
    order = np.argsort(pred, axis=1, kind="stable")
    srt = np.take_along_axis(pred, order, 1)
    new = np.ones_like(srt, dtype=bool)
    new[:, 1:] = srt[:, 1:] != srt[:, :-1]
    out = np.empty_like(new)
    np.put_along_axis(out, order, new, 1)
    return out


def kpis(pred, test_ur, test_u, cutoffs, metrics, item_num, item_pop=None, i_categories=None):
    """-> (per_user {name: float64 [nc, n]}, means {name: float64 [nc]} with 'coverage' among them when asked,
    coverage counts int64 [nc] or None).  Sums run in the order the reference's text gives: ascending position (map,
    dcg), ascending item id (popularity), (i, j) with i outer (diversity); np.cumsum adds one term after the other."""
    pred = np.asarray(pred).astype(np.int64)
    n, K = pred.shape
    nc = len(cutoffs)
    per = {m: np.zeros((nc, n)) for m in metrics if m != "coverage"}
    need_r = any(m in metrics for m in PER_USER[:9])
    if need_r:
        r, glen = hit_matrix(pred, test_ur, test_u, item_num)
        cum = np.cumsum(r, axis=1)
        pos1 = np.arange(1, K + 1, dtype=np.float64)
        disc = 1 / np.log2(np.arange(2, K + 2))
        cumdisc = np.concatenate([[0.0], np.cumsum(disc)])
        map_run = np.cumsum(np.where(r, cum / pos1, 0.0), axis=1)
        dcg_run = np.cumsum(np.where(r, disc, 0.0), axis=1)
        auc_run = np.cumsum(np.where(~r, cum, 0), axis=1)
        first = np.where(r.any(axis=1), r.argmax(axis=1), K)
    if "popularity" in metrics:
        by_id = np.argsort(pred, axis=1, kind="stable")
        pos_sorted = by_id
        ids_sorted = np.take_along_axis(pred, by_id, 1)
        keep_sorted = np.take_along_axis(r & first_occurrence(pred), by_id, 1)
    if "diversity" in metrics:
        cats = np.asarray(i_categories)[pred]                                   # [n, K, C]
        dist = np.sqrt((cats[:, :, None, :] != cats[:, None, :, :]).sum(-1).astype(np.float64))
    cover = np.zeros(nc, dtype=np.int64) if "coverage" in metrics else None
    with np.errstate(invalid="ignore", divide="ignore"):
        for c, k in enumerate(cutoffs):
            if need_r:
                h = cum[:, k - 1].astype(np.float64)
                pre, rec = h / k, h / glen
            for m in per:
                if m == "precision":
                    v = pre
                elif m == "recall":
                    v = rec
                elif m == "hit":
                    v = (h > 0).astype(np.float64)
                elif m == "mrr":
                    v = np.where(first < k, 1 / (first + 1.0), 0.0)
                elif m == "map":
                    v = np.where(h > 0, map_run[:, k - 1] / np.where(h > 0, h, 1), 0.0)
                elif m == "ndcg":
                    idcg = cumdisc[h.astype(np.int64)]
                    v = np.where(idcg != 0, dcg_run[:, k - 1] / np.where(idcg != 0, idcg, 1), 0.0)
                elif m == "f1":
                    v = 2 * pre * rec / (pre + rec)
                elif m == "auc":
                    v = auc_run[:, k - 1] / (h * (k - h))
                elif m == "popularity":
                    terms = np.where(keep_sorted & (pos_sorted < k), np.asarray(item_pop, dtype=np.float64)[ids_sorted], 0.0)
                    v = np.where(h > 0, np.cumsum(terms, axis=1)[:, -1] / glen, 0.0)
                elif m == "diversity":
                    iu, ju = np.triu_indices(k, 1)
                    v = (np.cumsum(dist[:, iu, ju], axis=1)[:, -1] / iu.size) if iu.size else np.full(n, np.nan)
                per[m][c] = v
            if cover is not None:
                cover[c] = np.unique(pred[:, :k]).size
        means = {m: v.mean(axis=1) for m, v in per.items()}
    if cover is not None:
        means["coverage"] = cover / item_num
    return per, means, cover


# ---- regimes ---------------------------------------------------------------------------------------------------------
def terms_of(metric, k, int_pop):
    """m of the module docstring: 0 = bitwise"""
    if metric in BITWISE or (metric == "popularity" and int_pop):
        return 0.0
    if metric == "f1":
        return 1.0
    return k * (k - 1) / 2.0 if metric == "diversity" else float(k)


def check_regimes(got_per, got_means, ref_per, ref_means, cutoffs, int_pop, what=""):
    """AssertionError unless (got_per, got_means) agree with the reference's values under the module's regimes.  got_per
    may lack metrics (then only their means are checked) or be None."""
    for m, ref in ref_per.items():
        ref = np.asarray(ref)
        for c, k in enumerate(cutoffs):
            v = ref[c]
            t = terms_of(m, k, int_pop)
            tol_user = 4 * t * U64 * np.abs(v)
            if got_per is not None and m in got_per:
                g = np.asarray(got_per[m])[c]
                assert np.array_equal(np.isnan(g), np.isnan(v)), f"{what}{m}@{k}: NaN pattern"
                ok = ~np.isnan(v)
                d = np.abs(g[ok] - v[ok])
                assert np.all(d <= tol_user[ok]), \
                    f"{what}{m}@{k}: per-list |d| up to {d.max():.3e}, bound {tol_user[ok][d.argmax()]:.3e} (m = {t})"
            gm, rm = float(np.asarray(got_means[m])[c]), float(np.asarray(ref_means[m])[c])
            if np.isnan(v).any():
                assert np.isnan(gm) and np.isnan(rm), f"{what}mean {m}@{k}: NaN expected, got {gm} / reference {rm}"
                continue
            tol = 0.0 if m == "hit" else 4 * v.size * U64 * np.abs(v).mean() + tol_user.mean()
            assert abs(gm - rm) <= tol, f"{what}mean {m}@{k}: |d| = {abs(gm - rm):.3e}, bound {tol:.3e}"
