#!/usr/bin/env python
"""Golden vectors for SLiM, generated from the REAL reference (`daisy.model.SLiMRecommender.SLiM`, imported from the
reference checkout, with scikit-learn's ElasticNet behind it; nothing is copied).  Runs only where the reference exists;
the output is committed:

    python tests/golden/make_golden_slim.py                 # -> tests/golden/kat_slim.npz
    python tests/golden/make_golden_slim.py --time-ml100k   # only times the reference's SLiM.fit at ml-100k's shape

Per fixture X of tests/slim_oracle.py::FIXTURES (tag_*): the (user, item, rating) triples; the reference's dense
w_sparse under np.random.seed(2022) (it visits the coordinates in random order); fixed candidates (30 per user, see
`candidates`), the reference's rank lists and A_tilde at them; the reference's sweep count per column (ref_iters); W*, the cyclic oracle at tol = 1e-12, max_iter = 5000, truncated; ref_dist =
max |W_ref - W*| and oracle_dist = max |W_oracle(default rule) - W*|, both over the common support.  The script asserts
that the three matrices have identical support: if a library update breaks that for a fixture, change that fixture's
seed, not the check.
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
from daisy.model.SLiMRecommender import SLiM  # noqa: E402

import scipy.sparse as sp  # noqa: E402

import slim_oracle as O  # noqa: E402

if not hasattr(sp.lil_matrix, "A"):        # SLiMRecommender.py:135,144 use the `.A` shorthand current scipy dropped
    sp.lil_matrix.A = property(lambda self: self.toarray())

N_CANDS = 30


def slim_config(U, I, alpha, elastic, topk):
    cfg = G.base_config()
    cfg.update(algo_name="slim", alpha=alpha, elastic=elastic, topk=topk, user_num=U, item_num=I)
    return cfg


class _Batch:
    """what SLiM.rank needs of a loader's tensors: .numpy() - as an array that owns its memory (scipy's fancy indexing of
    the lil matrix refuses the views torch hands out)"""

    def __init__(self, a):
        self._a = np.array(a)

    def numpy(self):
        return self._a.copy()


def reference_fit(u, i, r, U, I, alpha, elastic, topk):
    import warnings
    np.random.seed(2022)
    m = SLiM(slim_config(U, I, alpha, elastic, topk))
    m.ref_iters = []                               # scikit-learn's sweep count of every column's fit
    md_fit = m.md.fit

    def counted_fit(*a, **k):
        out = md_fit(*a, **k)
        m.ref_iters.append(int(m.md.n_iter_))
        return out
    m.md.fit = counted_fit
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")            # ConvergenceWarning of the columns that hit max_iter
        m.fit(pd.DataFrame({"user": u, "item": i, "rating": r}), verbose=False)
    return m


def candidates(A, rng):
    """N_CANDS distinct candidates per user in random order, drawn from the items the reference scores non-zero for the
    user; zero-score items only fill up a user with fewer.  The reference ranks with numpy's default argsort, which is not
    stable: the order of exact ties - in practice the zero scores - is an accident of the sort's implementation (and of the
    CPU's vector width), so lists that are to be compared position by position keep ties out of the ranked part."""
    U, I = A.shape
    out = np.zeros((U, N_CANDS), dtype=np.int64)
    for u in range(U):
        nz, z = np.nonzero(A[u])[0], np.nonzero(A[u] == 0)[0]
        take = rng.permutation(nz)[:N_CANDS]
        if len(take) < N_CANDS:
            take = np.concatenate([take, rng.permutation(z)[:N_CANDS - len(take)]])
        out[u] = rng.permutation(take)
    return out


def make_fixture(tag, out):
    U, I, dens, alpha, elastic, topk, seed, binary = O.FIXTURES[tag]
    u, i, r = O.fixture(U, I, dens, seed, binary)
    m = reference_fit(u, i, r, U, I, alpha, elastic, topk)
    W_ref = np.asarray(m.w_sparse.todense(), dtype=np.float32)
    cands = candidates(np.asarray(m.A_tilde.todense()), np.random.RandomState(1000 + seed))
    loader = [(_Batch(np.arange(U)), _Batch(cands))]
    ranks = np.asarray(m.rank(loader))
    a_cands = np.asarray(m.A_tilde[np.arange(U)[:, None], cands].todense(), dtype=np.float64)

    Gm = O.gram(O.dense(u, i, r, U, I))
    W_star = O.fit(Gm, U, alpha, elastic, topk, tol=1e-12, max_iter=5000)[0]
    W_def, sweeps, _, _ = O.fit(Gm, U, alpha, elastic, topk)
    assert np.array_equal(W_ref != 0, W_star != 0), f"{tag}: the reference's support differs from W*'s"
    assert np.array_equal(W_def != 0, W_star != 0), f"{tag}: the default rule's support differs from W*'s"
    sup = W_star != 0
    ref_dist = float(np.abs(W_ref.astype(np.float64) - W_star)[sup].max())
    oracle_dist = float(np.abs(W_def.astype(np.float64) - W_star)[sup].max())
    mine = O.rank_lists(O.scores(O.dense(u, i, r, U, I), W_def, np.arange(U), cands), cands, min(topk, N_CANDS))
    agree = float((mine == ranks).mean())
    print(f"{tag}: reference sweeps {min(m.ref_iters)}..{max(m.ref_iters)};", end=" ")
    print(f"{tag}: nnz(W) {int(sup.sum())}, empty columns {int((~sup.any(0)).sum())}, sweeps {sweeps[sweeps > 0].min()}.."
          f"{sweeps.max()}, ref_dist {ref_dist:.2e}, oracle_dist {oracle_dist:.2e}, rank agreement {agree:.4%}")
    out.update({f"{tag}_user": u.astype(np.int32), f"{tag}_item": i.astype(np.int32), f"{tag}_rating": r.astype(np.float32),
                f"{tag}_W_ref": W_ref, f"{tag}_W_star": W_star, f"{tag}_cands": cands, f"{tag}_rank_ref": ranks.astype(np.int64),
                f"{tag}_A_ref": a_cands, f"{tag}_ref_iters": np.asarray(m.ref_iters, dtype=np.int32), f"{tag}_ref_dist": np.float64(ref_dist), f"{tag}_oracle_dist": np.float64(oracle_dist)})


def time_ml100k():
    """the reference's SLiM.fit at ml-100k's shape (943 x 1682, 100 000 ratings 1..5, slim.yaml's alpha / elastic)"""
    rng = np.random.RandomState(0)
    U, I, n = 943, 1682, 100000
    pop = rng.zipf(1.3, I).clip(1, 50).astype(float)
    key = np.unique(rng.randint(0, U, 3 * n).astype(np.int64) * I + rng.choice(I, 3 * n, p=pop / pop.sum()))
    key = rng.permutation(key)[:n]
    u, i, r = key // I, key % I, rng.randint(1, 6, len(key)).astype(float)
    t0 = time.time()
    reference_fit(u, i, r, U, I, 1.0, 0.1, 50)
    print(f"reference SLiM.fit, {U} x {I}, {len(key)} ratings: {time.time() - t0:.1f} s on this host's CPU")


if __name__ == "__main__":
    if "--time-ml100k" in sys.argv:
        time_ml100k()
    else:
        out = {"tags": np.array(sorted(O.FIXTURES))}
        for tag in sorted(O.FIXTURES):
            make_fixture(tag, out)
        np.savez_compressed(os.path.join(HERE, "kat_slim.npz"), **out)
        print("wrote", os.path.join(HERE, "kat_slim.npz"))
