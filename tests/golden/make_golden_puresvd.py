#!/usr/bin/env python
"""Golden vectors for PureSVD, generated from the REAL reference (`daisy.model.PureSVDRecommender.PureSVD`, imported from
the reference checkout, with scikit-learn's randomized_svd behind it; nothing is copied).  Runs only where the reference
exists; the output is committed:

    python tests/golden/make_golden_puresvd.py                 # -> tests/golden/kat_puresvd.npz
    python tests/golden/make_golden_puresvd.py --time-ml100k   # only times the reference's PureSVD.fit at ml-100k's shape

Per fixture of tests/puresvd_oracle.py::FIXTURES (tag_*): the (user, item, rating) triples; the reference's sigma,
user_vec and item_vec (the leading rows only where a whole matrix would pass 128 KB: a committed file stays under 1 MiB);
fixed candidates (min(30, item_num) distinct items per user), the reference's scores and top-10 lists at them;
oracle_dev = max |scores(QR oracle) - scores(reference)| over ALL (user, item) pairs and oracle_vec_dev, the same for the
sign-flipped vectors (over the components puresvd_oracle.separated keeps: all of them but rankdef's null ones).  The tests' score tolerance is 100 x oracle_dev, their vector tolerance 100 x oracle_vec_dev.

The script asserts, for every ranked fixture, that the smallest gap between adjacent scores among each user's 11 best
reference candidate scores is >= 10^4 x that tolerance (so no row needs to be excluded from a list comparison), and
that no neighbouring singular values of a fixture are closer than 1e-6 sigma_0 (so no vector needs to be skipped).  If a
library update breaks that for a fixture, change that fixture's seed, not the check.
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
from daisy.model.PureSVDRecommender import PureSVD  # noqa: E402

import puresvd_oracle as O  # noqa: E402

N_CANDS, TOPK = 30, 10
VEC_DOUBLES = 16384            # rows * factors kept of user_vec / item_vec


def puresvd_config(U, I, factors, topk=TOPK):
    cfg = G.base_config()
    cfg.update(algo_name="puresvd", factors=factors, topk=topk, user_num=U, item_num=I)
    return cfg


class _Batch:
    """what PureSVD.rank needs of a loader's tensors: .numpy()"""

    def __init__(self, a):
        self._a = np.array(a)

    def numpy(self):
        return self._a.copy()


def reference_fit(u, i, r, U, I, factors):
    m = PureSVD(puresvd_config(U, I, factors))
    m.fit(pd.DataFrame({"user": u, "item": i, "rating": r}))
    return m


def candidates(U, I, rng):
    n = min(N_CANDS, I)
    return np.stack([rng.permutation(I)[:n] for _ in range(U)]).astype(np.int64)


def make_fixture(tag, out):
    U, I, factors, _, seed, ranked = O.FIXTURES[tag]
    u, i, r = O.triples(tag)
    X = O.dense(u, i, r, U, I)
    assert X.any(1).all(), f"{tag}: an empty user row"
    assert np.array_equal(X, X.astype(np.float32)), f"{tag}: a rating that fp32 does not hold"
    m = reference_fit(u, i, r, U, I, factors)
    user_vec, item_vec = np.asarray(m.user_vec, dtype=np.float64), np.asarray(m.item_vec, dtype=np.float64)
    sigma = np.linalg.norm(item_vec, axis=0)
    cands = candidates(U, I, np.random.RandomState(1000 + seed))
    users = np.arange(U)
    ranks = np.asarray(m.rank([(_Batch(users), _Batch(cands))]))
    sc = O.scores(user_vec, item_vec, users, cands)
    assert np.array_equal(ranks, O.rank_lists(sc, cands, TOPK)) or not ranked, f"{tag}: the stable lists differ"

    full_ref = user_vec @ item_vec.T
    devs = {}
    for name, norm in (("qr", O.qr_normalizer), ("cholqr2", O.cholqr2_normalizer)):
        f = O.fit(X, factors, norm)
        devs[name] = float(np.abs(f["user_vec"] @ f["item_vec"].T - full_ref).max())
        if name == "qr":
            ok = O.separated(sigma)
            oracle_vec_dev = float(max(np.abs(f["user_vec"] - user_vec)[:, ok].max(),
                                       np.abs(f["item_vec"] - item_vec)[:, ok].max()))
            n_iter, transposed = f["n_iter"], f["transposed"]
        else:
            dropped = f["dropped"]
    oracle_dev = devs["qr"]
    tol = 100.0 * oracle_dev
    gap = O.min_top_gap(sc)
    sgap = float(np.min(sigma[:-1] - sigma[1:]) / sigma[0])
    print(f"{tag}: {U} x {I}, k={factors}, n_iter={n_iter}, transposed={transposed}, dropped={dropped}, max|score| "
          f"{np.abs(full_ref).max():.2f}, oracle_dev {oracle_dev:.2e} (cholqr2 {devs['cholqr2']:.2e}), oracle_vec_dev "
          f"{oracle_vec_dev:.2e}, min top-11 gap {gap:.2e}, min sigma gap / sigma_0 {sgap:.2e}")
    if ranked:
        assert gap >= 1e4 * tol, f"{tag}: top-11 gap {gap:.2e} < 1e4 x tolerance {tol:.2e}: change the fixture's seed"
        assert ok.all(), f"{tag}: singular values closer than 1e-6 sigma_0: change the fixture's seed"
    rows = max(1, VEC_DOUBLES // factors)
    out.update({f"{tag}_user": u.astype(np.int32), f"{tag}_item": i.astype(np.int32), f"{tag}_rating": r.astype(np.float32),
                f"{tag}_sigma": sigma, f"{tag}_user_vec": user_vec[:rows], f"{tag}_item_vec": item_vec[:rows],
                f"{tag}_cands": cands, f"{tag}_scores_ref": sc, f"{tag}_rank_ref": ranks.astype(np.int64),
                f"{tag}_oracle_dev": np.float64(oracle_dev), f"{tag}_oracle_vec_dev": np.float64(oracle_vec_dev),
                f"{tag}_score_max": np.float64(np.abs(full_ref).max())})


def time_ml100k():
    """the reference's PureSVD.fit at ml-100k's shape (943 x 1682, 100 000 ratings 1..5, puresvd.yaml's 150 factors)"""
    rng = np.random.RandomState(0)
    U, I, n = 943, 1682, 100000
    pop = rng.zipf(1.3, I).clip(1, 50).astype(float)
    key = np.unique(rng.randint(0, U, 3 * n).astype(np.int64) * I + rng.choice(I, 3 * n, p=pop / pop.sum()))
    key = rng.permutation(key)[:n]
    u, i, r = key // I, key % I, rng.randint(1, 6, len(key)).astype(float)
    best = np.inf
    for _ in range(3):
        t0 = time.time()
        reference_fit(u, i, r, U, I, 150)
        best = min(best, time.time() - t0)
    print(f"reference PureSVD.fit, {U} x {I}, {len(key)} ratings, 150 factors: {best:.3f} s (best of 3) on this host's CPU")


if __name__ == "__main__":
    if "--time-ml100k" in sys.argv:
        time_ml100k()
    else:
        out = {"tags": np.array(sorted(O.FIXTURES))}
        for tag in sorted(O.FIXTURES):
            make_fixture(tag, out)
        np.savez_compressed(os.path.join(HERE, "kat_puresvd.npz"), **out)
        print("wrote", os.path.join(HERE, "kat_puresvd.npz"), os.path.getsize(os.path.join(HERE, "kat_puresvd.npz")), "bytes")
