"""EASE's numpy oracle (tests/ease_oracle.py) against the reference's golden vectors (tests/golden/kat_ease.npz, written by
tests/golden/make_golden_ease.py from the real daisy.model.EASERecommender.EASE): the Cholesky route reproduces the
reference's B and scores within 100 x the deviation the generator measured (the allowance tests/test_oracle_puresvd.py
gives its oracle: another BLAS may sum in another order than the generator's) and its top-10 lists exactly; the fixtures
keep the gap condition that makes a list comparison meaningful."""
import functools
import os

import numpy as np
import pytest

import ease_oracle as O
from conftest import GOLDEN, mf_config

TAGS = sorted(O.FIXTURES)
TOPK = 10


def ease_config(**over):
    cfg = mf_config(algo_name="ease", reg=200.0, topk=TOPK, user_num=3, item_num=4)
    cfg.update(over)
    return cfg


@functools.lru_cache(None)
def case(tag):
    """The fixture `tag` with its golden arrays: computed once, shared (read-only) by every test of the session."""
    k = np.load(os.path.join(GOLDEN, "kat_ease.npz"))
    U, I, reg, _, _ = O.FIXTURES[tag]
    u, i, r = k[f"{tag}_user"], k[f"{tag}_item"], k[f"{tag}_rating"]
    gu, gi, gr = O.triples(tag)
    assert np.array_equal(u, gu) and np.array_equal(i, gi) and np.array_equal(r, gr)      # the generator of the issue
    X = O.dense(u, i, r, U, I)
    c = dict(U=U, I=I, reg=reg, u=u, i=i, r=r, X=X, ranked=X.any(1), cands=k[f"{tag}_cands"], B=k[f"{tag}_B"],
             scores_ref=k[f"{tag}_scores_ref"], rank_ref=k[f"{tag}_rank_ref"], score_max=float(k[f"{tag}_score_max"]),
             tol=100.0 * float(k[f"{tag}_oracle_dev"]), B_tol=100.0 * float(k[f"{tag}_oracle_B_dev"]))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(None)
def oracle_B(tag):
    c = case(tag)
    B = O.fit(c["X"], c["reg"])
    B.setflags(write=False)
    return B


def test_golden_fixtures_are_what_the_issue_lists():
    shapes = {"tiny": (40, 23, 200.0), "ragged": (120, 97, 200.0), "oneplus": (30, 65, 10.0), "blocks": (300, 257, 200.0),
              "wide": (64, 130, 0.5), "dup": (50, 40, 200.0)}
    assert TAGS == sorted(shapes)
    for tag in TAGS:
        c = case(tag)
        assert (c["U"], c["I"], c["reg"]) == shapes[tag]
        assert c["cands"].shape == (c["U"], min(30, c["I"])) and c["rank_ref"].shape == (c["U"], TOPK)
        assert all(len(set(row)) == len(row) for row in c["cands"].tolist())
        assert c["B"].shape[1] == c["I"] and 1 <= c["B"].shape[0] <= c["I"] and c["B"].nbytes <= 128 << 10
        assert np.array_equal(c["X"], np.round(c["X"])) and 1 <= c["r"].min() and c["r"].max() <= 5
        # the ranges the issue measured: oracle_dev 9e-16 .. 1.2e-14, oracle_B_dev 1e-16 .. 1e-13, scores 2 .. 5
        assert 5e-16 < c["tol"] / 100 < 5e-14, f"{tag}: oracle_dev {c['tol'] / 100:.2e}"
        assert 5e-17 < c["B_tol"] / 100 < 5e-13, f"{tag}: oracle_B_dev {c['B_tol'] / 100:.2e}"
        assert 2.0 <= c["score_max"] <= 5.5
    d = case("dup")
    assert (~d["ranked"]).sum() == 1 and not d["ranked"][O.DUP_EMPTY_USER] and not d["X"][:, O.DUP_UNRATED_ITEM].any()
    assert len(np.unique(d["u"].astype(np.int64) * d["I"] + d["i"])) < len(d["u"])           # duplicate pairs
    assert d["X"].max() > 5                                                                 # ... that were summed
    assert all(case(t)["ranked"].all() for t in TAGS if t != "dup")
    w = case("wide")
    assert np.linalg.matrix_rank(w["X"]) < w["I"]                                           # X^T X alone is singular


@pytest.mark.parametrize("tag", TAGS)
def test_gap_condition_holds_from_the_stored_arrays(tag):
    c = case(tag)
    gap = O.min_top_gap(c["scores_ref"][c["ranked"]])
    print(f"{tag}: min top-11 gap {gap:.2e} = {gap / c['tol']:.1e} x tolerance")
    assert gap >= 1e4 * c["tol"]
    assert np.array_equal(O.rank_lists(c["scores_ref"], c["cands"], TOPK), c["rank_ref"])
    assert not c["scores_ref"][~c["ranked"]].any()
    assert np.array_equal(c["rank_ref"][~c["ranked"]], c["cands"][~c["ranked"]][:, :TOPK])


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_matches_the_reference(tag):
    c, B = case(tag), oracle_B(tag)
    rows = c["B"].shape[0]
    bdev = np.abs(B[:rows] - c["B"]).max()
    users = np.arange(c["U"])
    sc = O.scores(c["X"], B, users, c["cands"])
    dev = np.abs(sc - c["scores_ref"]).max()
    print(f"{tag}: max |B - reference| {bdev:.2e} = {bdev / (c['B_tol'] / 100):.2f} x oracle_B_dev, max |score - reference| "
          f"{dev:.2e} = {dev / (c['tol'] / 100):.2f} x oracle_dev")
    assert bdev <= c["B_tol"] and dev <= c["tol"]
    assert not np.diag(B).any()
    assert np.array_equal(O.rank_lists(sc, c["cands"], TOPK), c["rank_ref"])
    assert not sc[~c["ranked"]].any()                       # the user without history: exactly 0 everywhere


def test_spd_inverse_and_weights():
    rng = np.random.RandomState(0)
    M = rng.standard_normal((60, 40))
    A = M.T @ M + np.eye(40)
    P = O.spd_inverse(A)
    ref = np.linalg.inv(A)
    assert np.abs(A @ P - np.eye(40)).max() <= 100 * np.abs(A @ ref - np.eye(40)).max()
    assert np.array_equal(P, P.T) or np.abs(P - P.T).max() < 1e-15
    B = O.weights(P)
    assert not np.diag(B).any() and np.allclose(B[3, 5], -P[3, 5] / P[5, 5], rtol=0, atol=0)
