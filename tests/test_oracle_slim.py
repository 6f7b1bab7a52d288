"""SLiM's numpy oracle (tests/slim_oracle.py) against the reference's golden vectors (tests/golden/kat_slim.npz, written
by tests/golden/make_golden_slim.py from the real daisy.model.SLiMRecommender.SLiM): the cyclic descent at the default
stopping rule reaches the reference's support and lies within the triangle-inequality bound through the unique minimiser
W*; the rank lists agree with the reference's; the truncation quirk; the stopping decisions are not fragile."""
import functools
import os

import numpy as np
import pytest

import slim_oracle as O
from conftest import GOLDEN, mf_config

TAGS = sorted(O.FIXTURES)
RULES = {"default": (1e-4, 100), "tight": (1e-9, 2000)}


def slim_config(**over):
    cfg = mf_config(algo_name="slim", alpha=1.0, elastic=0.1, topk=50, user_num=3, item_num=4)
    cfg.update(over)
    return cfg


@functools.lru_cache(None)
def case(tag):
    """The fixture `tag` with its golden arrays: computed once, shared (read-only) by every test of the session."""
    k = np.load(os.path.join(GOLDEN, "kat_slim.npz"))
    U, I, dens, alpha, elastic, topk, seed, binary = O.FIXTURES[tag]
    u, i, r = k[f"{tag}_user"], k[f"{tag}_item"], k[f"{tag}_rating"]
    gu, gi, gr = O.fixture(U, I, dens, seed, binary)
    assert np.array_equal(u, gu) and np.array_equal(i, gi) and np.array_equal(r, gr)      # the generator of the issue
    X = O.dense(u, i, r, U, I)
    c = dict(U=U, I=I, alpha=alpha, elastic=elastic, topk=topk, u=u, i=i, r=r, X=X, G=O.gram(X), cands=k[f"{tag}_cands"],
             W_ref=k[f"{tag}_W_ref"], W_star=k[f"{tag}_W_star"], rank_ref=k[f"{tag}_rank_ref"], A_ref=k[f"{tag}_A_ref"],
             ref_iters=k[f"{tag}_ref_iters"],
             ref_dist=float(k[f"{tag}_ref_dist"]), oracle_dist=float(k[f"{tag}_oracle_dist"]))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(None)
def oracle_fit(tag, rule="default"):
    """(W, sweeps, gaps, kept columns, stopping margins) of the oracle on the fixture's exact G."""
    c = case(tag)
    margins = []
    tol, max_iter = RULES[rule]
    W, sweeps, gaps, kept = O.fit(c["G"], c["U"], c["alpha"], c["elastic"], c["topk"], tol, max_iter, infos=margins)
    W.setflags(write=False)
    return W, sweeps, gaps, kept, np.asarray(margins)


@functools.lru_cache(None)
def oracle_ranks(tag):
    c = case(tag)
    W = oracle_fit(tag)[0]
    sc = O.scores(c["X"], W, np.arange(c["U"]), c["cands"])
    return sc, O.rank_lists(sc, c["cands"], min(c["topk"], c["cands"].shape[1]))


@pytest.mark.parametrize("tag", TAGS)
def test_default_rule_against_the_reference(tag):
    c = case(tag)
    W = oracle_fit(tag)[0]
    assert np.array_equal(W != 0, c["W_ref"] != 0)
    dist = np.abs(W.astype(np.float64) - c["W_ref"].astype(np.float64)).max()
    print(f"{tag}: max |W_oracle - W_ref| = {dist:.3e}, bound {c['ref_dist'] + c['oracle_dist']:.3e}")
    # |W_oracle - W_ref| <= |W_ref - W*| + |W_oracle - W*|: both terms measured when the golden was written
    assert dist <= c["ref_dist"] + c["oracle_dist"]
    assert np.abs(W.astype(np.float64) - c["W_star"])[c["W_star"] != 0].max() <= c["oracle_dist"] * (1 + 1e-12)


def test_fixtures_cover_what_they_are_for():
    a, cc = case("A"), case("C")
    nz = (a["W_ref"] != 0).sum(0)
    assert nz.max() < a["topk"] and (nz == 0).any() and (np.diag(a["G"]) == 0).any()     # A: nz <= topk everywhere, an empty column
    # A: nz <= topk in the oracle's w BEFORE truncation (a column keeps nz - 1 entries), so every column drops its smallest
    assert max(len(rows) + 1 for rows, _ in oracle_fit("A")[3]) <= a["topk"]
    assert any(len(rows) for rows, _ in oracle_fit("A")[3])
    # C: more than one 256-coordinate block; the columns on which the reference runs all max_iter = 100 sweeps are the
    # unrated ones (yy == 0: its gap never drops below tol * yy = 0), which the oracle and the device leave at once; with
    # the cyclic order no rated column of the fixtures needs more than a few dozen sweeps
    assert cc["I"] > 256
    unrated = np.diag(cc["G"]) == 0
    assert unrated.any() and np.array_equal(cc["ref_iters"] == 100, unrated)
    assert (oracle_fit("C")[1][unrated] == 0).all() and (oracle_fit("C")[1][~unrated] > 0).all()
    assert oracle_fit("C", "tight")[1].max() > oracle_fit("C")[1].max()
    assert ((case("B")["W_star"] != 0).sum(0) == case("B")["topk"]).any()                 # B: columns cut at topk


@pytest.mark.parametrize("tag", TAGS)
def test_rank_lists_against_the_reference(tag):
    c = case(tag)
    sc, lists = oracle_ranks(tag)
    assert lists.shape == c["rank_ref"].shape
    # The golden candidates come from the items the reference scores non-zero for the user, because its unstable argsort
    # orders exact ties (the zero scores) by an accident of numpy's sort.  A user with fewer than 30 such items (fixture
    # A) is filled up with zero-score items: where those reach the ranked part, the agreement below also rests on how
    # the ties fell in the reference run that wrote the golden.
    agree = (lists == c["rank_ref"]).mean()
    print(f"{tag}: rank positions equal to the reference's: {agree:.4%}")
    assert agree >= 0.99
    # the reference's scores at the candidates: float64 products of its own W, so only W's distance separates them
    assert np.abs(sc.astype(np.float64) - c["A_ref"]).max() <= 5 * c["topk"] * (c["ref_dist"] + c["oracle_dist"]) + 1e-5


def test_truncation_quirk():
    rows, vals = O.truncate(np.zeros(5), 3)                                   # nz = 0
    assert rows.size == 0 and vals.size == 0
    rows, vals = O.truncate(np.array([0, 0, .7, 0, 0]), 3)                    # nz = 1: min(0, topk) = 0 kept
    assert rows.size == 0
    rows, vals = O.truncate(np.array([.2, 0, .7, .1, 0]), 3)                  # nz = 3 <= topk: the smallest is dropped
    assert rows.tolist() == [2, 0] and vals.tolist() == [np.float32(.7), np.float32(.2)]
    rows, vals = O.truncate(np.array([.2, .5, .7, .1, .3]), 3)                # nz = 5 > topk
    assert rows.tolist() == [2, 1, 4] and vals.dtype == np.float32 and rows.dtype == np.int32
    rows, vals = O.truncate(np.array([.5, .2, .5, .5, .1]), 2)                # ties: the lower row first
    assert rows.tolist() == [0, 2]


def test_cd_column_small_literals():
    """two items always rated together: column 0's coefficient of item 1 in closed form; an unrated item is skipped"""
    X = np.array([[1., 1., 0.], [1., 1., 0.], [0., 0., 0.]])
    G = O.gram(X)
    w, sweeps, gap = O.cd_column(G, 0, 3, 0.1, 0.5)
    a, b = 0.1 * 0.5 * 3, 0.1 * 0.5 * 3
    assert w[0] == 0 and w[2] == 0 and w[1] == (2.0 - a) / (2.0 + b) and sweeps >= 1 and gap < 1e-4 * 2.0
    w, sweeps, gap = O.cd_column(G, 2, 3, 0.1, 0.5)
    assert not w.any() and sweeps == 0


@pytest.mark.parametrize("rule", sorted(RULES))
def test_stopping_decisions_are_not_fragile(rule):
    """The device path sums the gap's terms in another order: a fixture whose stopping comparison sat within 1e-9
    (relative) of its threshold could stop a sweep apart.  (Reseed such a fixture.)"""
    for tag in TAGS:
        margins = oracle_fit(tag, rule)[4]
        print(f"{tag} {rule}: smallest stopping margin {margins.min():.3e}")
        assert margins.min() > 1e-9
