#!/usr/bin/env python
"""Golden vectors for EASE, generated from the REAL reference (`daisy.model.EASERecommender.EASE`, imported from the
reference checkout, with np.linalg.inv behind it; nothing is copied).  Runs only where the reference exists; the output
is committed:

    python tests/golden/make_golden_ease.py                 # -> tests/golden/kat_ease.npz
    python tests/golden/make_golden_ease.py --time-ml100k   # only times the reference's EASE.fit at ml-100k's shape

Per fixture of tests/ease_oracle.py::FIXTURES (tag_*): the (user, item, rating) triples; fixed candidates (min(30,
item_num) distinct items per user), the reference's scores at them (its predict: X[u, :] B[:, i]) and their top-10 lists in
stable order (see the note on the reference's `rank` in make_fixture); score_max; the leading rows of the
reference's B (up to 128 KB: a committed file stays under 1 MiB); oracle_dev = max |scores(oracle) - scores(reference)|
over ALL (user, item) pairs and oracle_B_dev, the same over B.  The tests' score tolerance is 100 x oracle_dev, their
tolerance on B 100 x oracle_B_dev: the oracle and the device take the inverse by the Cholesky route, the reference by LU,
and the device's sums run in another order than LAPACK's.

The script asserts, for every ranked user (all but the one without history in 'dup', whose scores are all exactly 0), that
the smallest gap between adjacent scores among the user's 11 best reference candidate scores is >= 10^4 x the score
tolerance.  If a library update breaks that for a fixture, change that fixture's seed, not the check.
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
from daisy.model.EASERecommender import EASE  # noqa: E402

import ease_oracle as O  # noqa: E402

N_CANDS, TOPK = 30, 10
B_DOUBLES = 16384              # rows * item_num kept of B


def ease_config(U, I, reg, topk=TOPK):
    cfg = G.base_config()
    cfg.update(algo_name="ease", reg=reg, topk=topk, user_num=U, item_num=I)
    return cfg


class _Batch:
    """what EASE.rank needs of a loader's tensors: .numpy()"""

    def __init__(self, a):
        self._a = np.array(a)

    def numpy(self):
        return self._a.copy()


def reference_fit(u, i, r, U, I, reg):
    cfg = ease_config(U, I, reg)
    m = EASE(cfg)
    m.fit(pd.DataFrame({cfg["UID_NAME"]: u, cfg["IID_NAME"]: i, cfg["INTER_NAME"]: r}))
    return m


def candidates(U, I, rng):
    n = min(N_CANDS, I)
    return np.stack([rng.permutation(I)[:n] for _ in range(U)]).astype(np.int64)


def make_fixture(tag, out):
    U, I, reg, _, seed = O.FIXTURES[tag]
    u, i, r = O.triples(tag)
    X = O.dense(u, i, r, U, I)
    ranked = X.any(1)
    if tag == "dup":
        assert not ranked[O.DUP_EMPTY_USER] and ranked.sum() == U - 1 and not X[:, O.DUP_UNRATED_ITEM].any()
        assert len(np.unique(u.astype(np.int64) * I + i)) < len(u), "dup: no duplicate pair"
    else:
        assert ranked.all(), f"{tag}: an empty user row"
    assert np.array_equal(X, np.round(X)) and X.max() * X.max() * U < 2 ** 24, f"{tag}: G is not exact in fp32"
    m = reference_fit(u, i, r, U, I, reg)
    B_ref = np.asarray(m.item_similarity, dtype=np.float64)
    assert B_ref.shape == (I, I) and m.interaction_matrix.dtype == np.float32
    assert np.array_equal(np.asarray(m.interaction_matrix.todense(), dtype=np.float64), X)
    cands = candidates(U, I, np.random.RandomState(1000 + seed))
    users = np.arange(U)
    # the scores of the reference's predict / full_rank (EASERecommender.py:50, 70): X[u, :] B[:, i]
    sc = O.scores(X, B_ref, users, cands)
    for uu in (0, U // 2, U - 1):
        assert abs(m.predict(uu, int(cands[uu, 0])) - sc[uu, 0]) <= 1e-12 * max(1.0, abs(sc[uu, 0])), f"{tag}: predict"
        if ranked[uu]:
            full = X[uu] @ B_ref
            assert np.array_equal(np.asarray(m.full_rank(uu)).reshape(-1), np.argsort(-full, kind="stable")[:TOPK]), \
                f"{tag}: full_rank"
    ranks = O.rank_lists(sc, cands, TOPK)
    # EASERecommender.py:60 gathers item_similarity[cands_ids, :]: the reference's `rank` scores a candidate c by
    # X[u, :] B[c, :] - B TRANSPOSED against its own predict and full_rank.  Confirmed here; daisyrec_amd ranks by the
    # scores of predict / full_rank (deviations), and the lists stored are the stable order of those.
    written = np.asarray(m.rank([(_Batch(users), _Batch(cands))]))
    assert np.array_equal(written[ranked], O.rank_lists(O.scores(X, B_ref.T, users, cands), cands, TOPK)[ranked]), \
        f"{tag}: the reference's rank is not the transposed product either"
    assert not sc[~ranked].any()

    B_or = O.fit(X, reg)
    oracle_B_dev = float(np.abs(B_or - B_ref).max())
    oracle_dev = float(np.abs(X @ B_or - X @ B_ref).max())
    tol = 100.0 * oracle_dev
    gap = O.min_top_gap(sc[ranked])
    cond = np.linalg.cond(O.system(X, reg))
    print(f"{tag}: {U} x {I}, reg={reg}, cond(A) {cond:.1e}, max|score| {np.abs(X @ B_ref).max():.2f}, oracle_dev "
          f"{oracle_dev:.2e}, oracle_B_dev {oracle_B_dev:.2e}, min top-11 gap {gap:.2e} = {gap / tol:.1e} x tolerance")
    assert oracle_dev > 0 and oracle_B_dev > 0
    assert gap >= 1e4 * tol, f"{tag}: top-11 gap {gap:.2e} < 1e4 x tolerance {tol:.2e}: change the fixture's seed"
    rows = max(1, min(I, B_DOUBLES // I))
    out.update({f"{tag}_user": u.astype(np.int32), f"{tag}_item": i.astype(np.int32), f"{tag}_rating": r.astype(np.float32),
                f"{tag}_cands": cands, f"{tag}_scores_ref": sc, f"{tag}_rank_ref": ranks.astype(np.int64),
                f"{tag}_B": B_ref[:rows], f"{tag}_oracle_dev": np.float64(oracle_dev),
                f"{tag}_oracle_B_dev": np.float64(oracle_B_dev), f"{tag}_score_max": np.float64(np.abs(X @ B_ref).max())})


def time_ml100k():
    """the reference's EASE.fit at ml-100k's shape (943 x 1682, 100 000 ratings 1..5, ease.yaml's reg = 200)"""
    rng = np.random.RandomState(0)
    U, I, n = 943, 1682, 100000
    pop = rng.zipf(1.3, I).clip(1, 50).astype(float)
    key = np.unique(rng.randint(0, U, 3 * n).astype(np.int64) * I + rng.choice(I, 3 * n, p=pop / pop.sum()))
    key = rng.permutation(key)[:n]
    u, i, r = key // I, key % I, rng.randint(1, 6, len(key)).astype(float)
    best = np.inf
    for _ in range(3):
        t0 = time.time()
        reference_fit(u, i, r, U, I, 200.0)
        best = min(best, time.time() - t0)
    print(f"reference EASE.fit, {U} x {I}, {len(key)} ratings, reg 200: {best:.3f} s (best of 3) on this host's CPU")


if __name__ == "__main__":
    if "--time-ml100k" in sys.argv:
        time_ml100k()
    else:
        out = {"tags": np.array(sorted(O.FIXTURES))}
        for tag in sorted(O.FIXTURES):
            make_fixture(tag, out)
        np.savez_compressed(os.path.join(HERE, "kat_ease.npz"), **out)
        print("wrote", os.path.join(HERE, "kat_ease.npz"), os.path.getsize(os.path.join(HERE, "kat_ease.npz")), "bytes")
