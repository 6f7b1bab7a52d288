#!/usr/bin/env python
"""Golden vectors for ItemKNN / UserKNN, generated from the REAL reference (`daisy.model.KNNCFRecommender`: ItemKNNCF,
UserKNNCF and Similarity, imported from the reference checkout; nothing is copied).  Runs only where the reference exists;
the output is committed:

    python tests/golden/make_golden_knn.py                 # -> tests/golden/kat_knn.npz
    python tests/golden/make_golden_knn.py --time-ml100k   # only times the reference's two fits at ml-100k's shape

Per fixture of tests/knn_oracle.py::FIXTURES (tag_*): the (user, item, rating) triples, the reference's W as (row, col,
val) triples and, by the fixture's regime (knn_oracle.py's docstring), what this script ASSERTS before it writes:

  'a'  the oracle's W and the reference's are bitwise equal;
  'b'  the patterns are equal, oracle_W_dev = max |W_oracle - W_ref| > 0 is stored, and in every column the K-th and the
       (K+1)-th largest candidate weight differ by >= 1e4 x (100 x oracle_W_dev): another summation order cannot flip the
       selection;
  'c'  per column the sorted kept values are bitwise equal, the ids agree for every entry strictly above the smallest kept
       value, every differing entry has that value, and at least one column does have such a boundary tie.

For 'a' and 'b' also: fixed candidates (min(30, item_num) distinct items per user), the reference's pred_mat at them,
oracle_dev = max |pred(W_oracle) - pred_mat| over all pairs, (|X| |W|) at the candidates (the fp64 summation bound of the
tests), the stable order of the reference's own scores, and the check that the reference's `rank` agrees with that order
for every user whose 11 best candidate scores are decided (adjacent scores differ by >= 1e4 x the score tolerance or are
both exactly 0; among candidates that score exactly 0 the reference's unstable argsort may permute, so there only the
scores of its ids are compared).  The mask of the decided users is stored.  The seeds of the 'a' fixtures are chosen so
that every user with history is decided; the 'b' fixtures cannot meet that (see make_fixture) and are small (40 x 8,
K = 2) because their K-th gap condition asks for gaps of some 6 % of a weight in every column.  If a check fails after a
library update, change the fixture's seed, not the check.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402  (puts the reference checkout and the logging shims on sys.path)

import pandas as pd  # noqa: E402
import scipy.sparse as sp  # noqa: E402

if not hasattr(sp.spmatrix, "A"):        # KNNCFRecommender.py:446, 455 (scipy >= 1.14 removed the alias of toarray())
    sp.spmatrix.A = property(lambda self: self.toarray())

from daisy.model.KNNCFRecommender import ItemKNNCF, Similarity, UserKNNCF  # noqa: E402

import knn_oracle as O  # noqa: E402


def knn_config(U, I, similarity, normalize, shrink, maxk, topk=O.TOPK):
    cfg = G.base_config()
    cfg.update(algo_name="itemknn", maxk=maxk, shrink=shrink, normalize=normalize, similarity=similarity, topk=topk,
               user_num=U, item_num=I)
    return cfg


class _Batch:
    def __init__(self, a):
        self._a = np.array(a)

    def numpy(self):
        return self._a.copy()


def reference_fit(model, u, i, r, U, I, similarity, normalize, shrink, maxk):
    """-> (the fitted reference model, its W as a dense float32 [n, n])"""
    cfg = knn_config(U, I, similarity, normalize, shrink, maxk)
    m = (ItemKNNCF if model == "item" else UserKNNCF)(cfg)
    df = pd.DataFrame({"user": u, "item": i, "rating": r})
    m.fit(df)
    # fit() does not keep W: the same Similarity call once more (KNNCFRecommender.py:422-429 / :500-507)
    train = sp.csc_matrix((list(df["rating"]), (list(df["user"]), list(df["item"]))), shape=(U, I))
    sim = Similarity(train if model == "item" else train.T, shrink=shrink, topK=maxk, normalize=normalize,
                     similarity=similarity, logger=cfg["logger"])
    W = sim.compute_similarity()
    assert W.dtype == np.float32
    return m, np.asarray(W.todense(), dtype=np.float32)


def candidates(U, I, rng):
    n = min(O.N_CANDS, I)
    return np.stack([rng.permutation(I)[:n] for _ in range(U)]).astype(np.int64)


def kth_gap(X, M, model, similarity, normalize, shrink, K):
    """the smallest difference, over the columns, between the K-th and the (K+1)-th largest candidate weight (oracle)"""
    D, Md = O.data_matrix(X, M, model)
    D = O.prepare(D, Md, similarity)
    Gm = (D.T @ D).astype(np.float32)
    Wr = O.weights(Gm, np.sqrt(np.diag(Gm)), O.mode_of(similarity, normalize), shrink).astype(np.float64)
    n = Wr.shape[0]
    if K >= n:
        return np.inf
    s = -np.sort(-Wr, axis=1)
    return float(np.min(s[:, K - 1] - s[:, K]))


def make_fixture(tag, out):
    model, U, I, similarity, normalize, shrink, K, _, seed, regime = O.FIXTURES[tag]
    u, i, r = O.triples(tag)
    X, M = O.dense(u, i, r, U, I)
    has = X.any(1)
    if tag == "cold":
        assert not has[O.COLD_EMPTY_USER] and has.sum() == U - 1 and not X[:, O.COLD_ITEM].any()
        assert len(np.unique(u.astype(np.int64) * I + i)) < len(u), "cold: no duplicate pair"
    else:
        assert has.all() and X.any(0).all(), f"{tag}: an empty row or column"
    m, W_ref = reference_fit(model, u, i, r, U, I, similarity, normalize, shrink, K)
    W_or = O.fit(X, M, model, similarity, normalize, shrink, K)
    n = W_ref.shape[0]
    assert W_or.shape == (n, n)
    rr, cc = np.nonzero(W_ref)
    out.update({f"{tag}_user": u.astype(np.int32), f"{tag}_item": i.astype(np.int32), f"{tag}_rating": r.astype(np.float32),
                f"{tag}_W_row": rr.astype(np.int16 if n < 32768 else np.int32),
                f"{tag}_W_col": cc.astype(np.int16 if n < 32768 else np.int32), f"{tag}_W_val": W_ref[rr, cc]})
    note = ""
    if regime == "a":
        assert np.array_equal(W_or.view(np.uint32), W_ref.view(np.uint32)), f"{tag}: W is not bitwise the reference's"
    elif regime == "b":
        assert np.array_equal(W_or != 0, W_ref != 0), f"{tag}: the patterns differ"
        w_dev = float(np.abs(W_or.astype(np.float64) - W_ref).max())
        gap = kth_gap(X, M, model, similarity, normalize, shrink, K)
        assert w_dev > 0, f"{tag}: oracle_W_dev is 0"
        assert gap >= 1e4 * 100 * w_dev, f"{tag}: K-th gap {gap:.2e} < 1e6 x oracle_W_dev {w_dev:.2e}: change the seed"
        out[f"{tag}_oracle_W_dev"] = np.float64(w_dev)
        note = f", oracle_W_dev {w_dev:.2e}, max|W| {np.abs(W_ref).max():.3f}, K-th gap {gap:.2e}"
    else:
        ties = 0
        for j in range(n):
            a, b = W_or[:, j], W_ref[:, j]
            va, vb = np.sort(a[a != 0]), np.sort(b[b != 0])
            assert np.array_equal(va.view(np.uint32), vb.view(np.uint32)), f"{tag}: column {j}: the kept values differ"
            if not len(va):
                continue
            lo = va[0]
            assert np.array_equal(np.where(a > lo, a, 0), np.where(b > lo, b, 0)), f"{tag}: column {j}: ids above the boundary"
            diff = a != b
            assert np.all((a[diff] == lo) | (a[diff] == 0)) and np.all((b[diff] == lo) | (b[diff] == 0)), f"{tag}: column {j}"
            ties += bool(diff.any())
        assert ties >= 1, f"{tag}: no column with a boundary tie: change the seed"
        note = f", {ties} of {n} columns keep other ids among boundary ties"
    if regime in "ab":
        P_ref = np.asarray(m.pred_mat.todense(), dtype=np.float64)
        assert P_ref.shape == (U, I)
        cands = candidates(U, I, np.random.RandomState(1000 + seed))
        sc = np.take_along_axis(P_ref, cands, 1)
        oracle_dev = float(np.abs(O.pred(X, W_or, model) - P_ref).max())
        absprod = O.abs_pred(X, W_ref, model)
        tol = max(100 * oracle_dev, K * 2.0 ** -52 * float(absprod.max()))
        dec = O.decided(sc, tol)
        # Regime 'b' cannot meet this for every user: its tolerance is 100 x an fp32 rounding error of W, and 1e4 x that asks
        # for gaps of some 6 % between all of a user's 11 best scores.  There the mask of the decided users is stored and
        # the lists are compared for those alone.
        assert regime == "b" or dec[has].all(), f"{tag}: users {np.nonzero(has & ~dec)[0]} are not decided: change the seed"
        out[f"{tag}_decided"] = dec
        note += f", {int(dec[has].sum())} of {int(has.sum())} users with history decided"
        topk = min(O.TOPK, cands.shape[1])
        ranks = O.rank_lists(sc, cands, topk)
        written = np.asarray(m.rank([(_Batch(np.arange(U)), _Batch(cands))]))
        assert written.shape == ranks.shape
        for uu in np.nonzero(dec)[0]:
            s_st = P_ref[uu, ranks[uu]]
            nz = s_st != 0
            assert np.array_equal(written[uu][nz], ranks[uu][nz]), f"{tag}: the reference's rank, user {uu}"
            assert np.array_equal(P_ref[uu, written[uu]], s_st), f"{tag}: the reference's rank scores, user {uu}"
        assert not sc[~has].any()
        for uu in (0, U // 2, U - 1):
            assert m.predict(uu, int(cands[uu, 0])) == sc[uu, 0]
        out.update({f"{tag}_cands": cands, f"{tag}_scores_ref": sc, f"{tag}_rank_ref": ranks.astype(np.int64),
                    f"{tag}_oracle_dev": np.float64(oracle_dev), f"{tag}_absprod": np.take_along_axis(absprod, cands, 1)})
        note += f", oracle_dev {oracle_dev:.2e}, max|score| {np.abs(P_ref).max():.2f}, score tolerance {tol:.2e}"
    print(f"{tag}: {model} {U} x {I}, {similarity}, normalize={normalize}, shrink={shrink}, K={K}, regime {regime}, "
          f"nnz(W) {len(rr)}{note}")


def ml100k_frame():
    """the synthetic set of make_golden_ease.py::time_ml100k: 943 x 1682, 100 000 ratings 1..5"""
    rng = np.random.RandomState(0)
    U, I, n = 943, 1682, 100000
    pop = rng.zipf(1.3, I).clip(1, 50).astype(float)
    key = np.unique(rng.randint(0, U, 3 * n).astype(np.int64) * I + rng.choice(I, 3 * n, p=pop / pop.sum()))
    key = rng.permutation(key)[:n]
    return U, I, key // I, key % I, rng.randint(1, 6, len(key)).astype(float)


def time_ml100k():
    U, I, u, i, r = ml100k_frame()
    df = pd.DataFrame({"user": u, "item": i, "rating": r})
    for name, cls in (("ItemKNNCF", ItemKNNCF), ("UserKNNCF", UserKNNCF)):
        best = np.inf
        for _ in range(3):
            m = cls(knn_config(U, I, "cosine", True, 100, 40))
            t0 = time.time()
            m.fit(df)
            best = min(best, time.time() - t0)
        print(f"reference {name}.fit, {U} x {I}, {len(u)} ratings, cosine, shrink 100, maxk 40: {best:.3f} s (best of 3) "
              "on this host's CPU")


if __name__ == "__main__":
    if "--time-ml100k" in sys.argv:
        time_ml100k()
    else:
        out = {"tags": np.array(sorted(O.FIXTURES))}
        for tag in O.FIXTURES:
            make_fixture(tag, out)
        path = os.path.join(HERE, "kat_knn.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path), "bytes")
