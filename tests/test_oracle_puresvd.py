"""PureSVD's numpy oracle (tests/puresvd_oracle.py) against the reference's golden vectors (tests/golden/kat_puresvd.npz,
written by tests/golden/make_golden_puresvd.py from the real daisy.model.PureSVDRecommender.PureSVD): with either
normaliser - Householder QR or Cholesky-QR2 with the dependent-column rule - the restated randomized_svd reproduces the
reference's scores within 100 x oracle_dev and its top-10 lists exactly; orientation, iteration count and the number of
dropped columns per orthonormalisation are what the fixtures were built to exercise."""
import functools
import os

import numpy as np
import pytest

import puresvd_oracle as O
from conftest import GOLDEN, mf_config

TAGS = sorted(O.FIXTURES)
RANKED = [t for t in TAGS if O.FIXTURES[t][5]]
NORMALIZERS = {"qr": O.qr_normalizer, "cholqr2": O.cholqr2_normalizer}
TOPK = 10
#               tag: (n_iter, transposed, dropped columns per orthonormalisation)
EXPECTED = {"zipf": (7, False, 0), "wide": (4, True, 0), "tiny": (4, False, 0), "fewitems": (4, False, 6),
            "rankdef": (4, False, 13), "default_r": (4, False, 0)}


def puresvd_config(**over):
    cfg = mf_config(algo_name="puresvd", factors=2, topk=TOPK, user_num=3, item_num=4)
    cfg.update(over)
    return cfg


@functools.lru_cache(None)
def case(tag):
    """The fixture `tag` with its golden arrays: computed once, shared (read-only) by every test of the session."""
    k = np.load(os.path.join(GOLDEN, "kat_puresvd.npz"))
    U, I, factors, _, _, ranked = O.FIXTURES[tag]
    u, i, r = k[f"{tag}_user"], k[f"{tag}_item"], k[f"{tag}_rating"]
    gu, gi, gr = O.triples(tag)
    assert np.array_equal(u, gu) and np.array_equal(i, gi) and np.array_equal(r, gr)      # the generator of the issue
    c = dict(U=U, I=I, factors=factors, ranked=ranked, u=u, i=i, r=r, X=O.dense(u, i, r, U, I), cands=k[f"{tag}_cands"],
             sigma=k[f"{tag}_sigma"], user_vec=k[f"{tag}_user_vec"], item_vec=k[f"{tag}_item_vec"],
             scores_ref=k[f"{tag}_scores_ref"], rank_ref=k[f"{tag}_rank_ref"], score_max=float(k[f"{tag}_score_max"]),
             tol=100.0 * float(k[f"{tag}_oracle_dev"]), vec_tol=100.0 * float(k[f"{tag}_oracle_vec_dev"]))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(None)
def oracle_fit(tag, normalizer):
    c = case(tag)
    f = O.fit(c["X"], c["factors"], NORMALIZERS[normalizer])
    for v in f.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return f


def test_golden_fixtures_are_what_the_issue_lists():
    assert TAGS == sorted(EXPECTED)
    for tag in TAGS:
        c = case(tag)
        assert c["X"].any(1).all(), f"{tag}: an empty user row"
        assert c["cands"].shape == (c["U"], min(30, c["I"])) and c["rank_ref"].shape == (c["U"], TOPK)
        assert 1e-15 < c["tol"] / 100 < 1e-12, f"{tag}: oracle_dev {c['tol'] / 100:.2e} outside the range the issue measured"
        if c["ranked"]:
            assert O.min_top_gap(c["scores_ref"]) >= 1e4 * c["tol"]
            assert O.separated(c["sigma"]).all()
    assert np.linalg.matrix_rank(case("rankdef")["X"]) == 5


@pytest.mark.parametrize("normalizer", sorted(NORMALIZERS))
@pytest.mark.parametrize("tag", TAGS)
def test_oracle_scores_and_lists_match_the_reference(tag, normalizer):
    c, f = case(tag), oracle_fit(tag, normalizer)
    users = np.arange(c["U"])
    sc = O.scores(f["user_vec"], f["item_vec"], users, c["cands"])
    dev = np.abs(sc - c["scores_ref"]).max()
    print(f"{tag}/{normalizer}: max |score - reference| {dev:.2e} = {dev / (c['tol'] / 100):.2f} x oracle_dev")
    assert dev <= c["tol"]
    assert np.abs(f["sigma"] - c["sigma"]).max() <= c["tol"] / c["score_max"] * c["sigma"][0]
    if c["ranked"]:
        assert np.array_equal(O.rank_lists(sc, c["cands"], TOPK), c["rank_ref"])
        rows = c["user_vec"].shape[0]
        assert np.abs(f["user_vec"][:rows] - c["user_vec"]).max() <= c["vec_tol"]
        assert np.abs(f["item_vec"][:c["item_vec"].shape[0]] - c["item_vec"]).max() <= c["vec_tol"]


@pytest.mark.parametrize("tag", TAGS)
def test_orientation_iterations_and_dropped_columns(tag):
    n_iter, transposed, dropped = EXPECTED[tag]
    f = oracle_fit(tag, "cholqr2")
    assert (f["n_iter"], f["transposed"]) == (n_iter, transposed)
    assert f["dropped"] == [dropped] * (2 * n_iter + 2)
    c = case(tag)
    if dropped:
        assert c["factors"] + O.OVERSAMPLES - dropped == np.linalg.matrix_rank(c["X"])


def test_cholqr2_on_a_dependent_column():
    rng = np.random.RandomState(0)
    Y = rng.standard_normal((50, 6))
    Y[:, 3] = Y[:, 0] - 2 * Y[:, 2]
    Q, R, dropped = O.cholqr2_normalizer(Y)
    assert dropped == 1 and not Q[:, 3].any() and not R[3].any() and R[:3, 3].any()
    keep = [0, 1, 2, 4, 5]
    assert np.abs(Q[:, keep].T @ Q[:, keep] - np.eye(5)).max() < 1e-14
    assert np.abs(Q @ R - Y).max() < 1e-13


def test_sign_rule_of_the_golden_vectors():
    for tag in RANKED:
        c = case(tag)
        if c["user_vec"].shape[0] < c["U"]:
            continue                          # only the leading rows are stored: the largest entry may lie below them
        uv = c["user_vec"]
        assert (uv[np.argmax(np.abs(uv), axis=0), np.arange(uv.shape[1])] > 0).all()
