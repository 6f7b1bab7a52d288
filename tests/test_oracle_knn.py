"""The numpy oracle of ItemKNN / UserKNN (tests/knn_oracle.py) against the reference's golden vectors (tests/golden/
kat_knn.npz, written by tests/golden/make_golden_knn.py from the real daisy.model.KNNCFRecommender): by the fixture's regime
W is reproduced bit for bit ('a'), within 100 x the deviation the generator measured and with the same pattern ('b'), or
with bitwise the same kept values per column and other ids only among boundary ties ('c'); the scores and the lists follow
for 'a' and 'b'."""
import functools
import os

import numpy as np
import pytest

import knn_oracle as O
from conftest import GOLDEN, mf_config

TAGS = list(O.FIXTURES)
SCORED = [t for t in TAGS if O.FIXTURES[t][9] in "ab"]
TOPK = O.TOPK


def knn_config(**over):
    cfg = mf_config(algo_name="itemknn", maxk=40, shrink=100, normalize=True, similarity="cosine", topk=TOPK, user_num=3,
                    item_num=4)
    cfg.update(over)
    return cfg


@functools.lru_cache(None)
def case(tag):
    """The fixture `tag` with its golden arrays: computed once, shared (read-only) by every test of the session."""
    k = np.load(os.path.join(GOLDEN, "kat_knn.npz"))
    model, U, I, sim, normalize, shrink, K, _, _, regime = O.FIXTURES[tag]
    u, i, r = k[f"{tag}_user"], k[f"{tag}_item"], k[f"{tag}_rating"]
    gu, gi, gr = O.triples(tag)
    assert np.array_equal(u, gu) and np.array_equal(i, gi) and np.array_equal(r, gr)
    X, M = O.dense(u, i, r, U, I)
    n = I if model == "item" else U
    W = np.zeros((n, n), dtype=np.float32)
    W[k[f"{tag}_W_row"].astype(np.int64), k[f"{tag}_W_col"].astype(np.int64)] = k[f"{tag}_W_val"]
    c = dict(tag=tag, model=model, U=U, I=I, n=n, sim=sim, normalize=normalize, shrink=shrink, K=K, regime=regime, u=u, i=i,
             r=r, X=X, M=M, has=X.any(1), W=W)
    if regime == "b":
        c["W_tol"] = 100.0 * float(k[f"{tag}_oracle_W_dev"])
    if regime in "ab":
        c.update(cands=k[f"{tag}_cands"], scores_ref=k[f"{tag}_scores_ref"], rank_ref=k[f"{tag}_rank_ref"],
                 decided=k[f"{tag}_decided"], oracle_dev=float(k[f"{tag}_oracle_dev"]), absprod=k[f"{tag}_absprod"])
        # the issue's score tolerance, per pair: 100 x oracle_dev, or the fp64 bound of a sum in another order
        c["tol"] = np.maximum(100.0 * c["oracle_dev"], K * 2.0 ** -52 * c["absprod"])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(None)
def oracle_W(tag):
    c = case(tag)
    W = O.fit(c["X"], c["M"], c["model"], c["sim"], c["normalize"], c["shrink"], c["K"])
    W.setflags(write=False)
    return W


def check_W(c, W, against_oracle=None):
    """W [n, n] float32 under the fixture's regime; regime 'c' with against_oracle: equal to that matrix exactly (the
    device follows the oracle's tie rule), else the tie-tolerant comparison with the reference"""
    W = np.asarray(W)
    assert W.dtype == np.float32 and W.shape == c["W"].shape
    ref = c["W"]
    if c["regime"] == "a":
        assert np.array_equal(W.view(np.uint32), ref.view(np.uint32))
    elif c["regime"] == "b":
        assert np.array_equal(W != 0, ref != 0)
        dev = np.abs(W.astype(np.float64) - ref).max()
        print(f"{c['tag']}: max |W - reference| {dev:.2e} = {dev / (c['W_tol'] / 100):.2f} x oracle_W_dev (allowed: 100)")
        assert dev <= c["W_tol"]
    elif against_oracle is not None:
        assert np.array_equal(W.view(np.uint32), np.asarray(against_oracle).view(np.uint32))
    else:
        ties = 0
        for j in range(c["n"]):
            a, b = W[:, j], ref[:, j]
            va, vb = np.sort(a[a != 0]), np.sort(b[b != 0])
            assert np.array_equal(va.view(np.uint32), vb.view(np.uint32)), j
            if len(va):
                lo = va[0]
                assert np.array_equal(np.where(a > lo, a, 0), np.where(b > lo, b, 0)), j
                diff = a != b
                assert np.all((a[diff] == lo) | (a[diff] == 0)) and np.all((b[diff] == lo) | (b[diff] == 0)), j
                ties += bool(diff.any())
        assert ties >= 1                                    # the tie rule is exercised


def check_scores(c, sc, ranks=None):
    """scores [U, C] at the fixture's candidates within the issue's tolerance; lists identical for the decided users with
    history, the first candidates for a user without history"""
    dev = np.abs(sc - c["scores_ref"])
    print(f"{c['tag']}: max |score - reference| {dev.max():.2e}, max of (deviation / tolerance) {np.max(dev / c['tol'].clip(1e-300)):.2e}")
    assert np.all(dev <= c["tol"])
    assert not sc[~c["has"]].any()
    if ranks is not None:
        sel = c["has"] & c["decided"]
        assert ranks.shape == c["rank_ref"].shape and np.array_equal(ranks[sel], c["rank_ref"][sel])
        assert np.array_equal(ranks[~c["has"]], c["cands"][~c["has"]][:, :ranks.shape[1]])


def test_golden_fixtures_are_what_the_issue_lists():
    ns = {case(t)["n"] for t in TAGS}
    assert {45, 255, 256, 257, 700} <= ns                   # (n = 1: the reference itself fails on one column)
    ks = {(case(t)["K"], case(t)["n"]) for t in TAGS}
    assert {k for k, _ in ks} >= {1, 7, 40} and any(k == n - 1 for k, n in ks) and any(k > n for k, n in ks)
    sims = {(case(t)["sim"], case(t)["normalize"], case(t)["shrink"]) for t in TAGS}
    assert {("cosine", True, 100), ("cosine", True, 0), ("asymmetric", True, 100), ("adjusted", True, 100),
            ("pearson", True, 100), ("jaccard", True, 0), ("dice", True, 0), ("tversky", True, 0), ("cosine", False, 0),
            ("cosine", False, 10)} <= sims
    u = case("user")
    assert (u["model"], u["U"], u["I"], u["n"]) == ("user", 40, 130, 40)
    d = case("cold")
    assert (~d["has"]).sum() == 1 and not d["has"][O.COLD_EMPTY_USER] and not d["X"][:, O.COLD_ITEM].any()
    assert len(np.unique(d["u"].astype(np.int64) * d["I"] + d["i"])) < len(d["u"]) and d["X"].max() > 5
    for t in TAGS:
        c = case(t)
        assert np.array_equal(c["X"], np.round(c["X"])) and 1 <= c["r"].min() and c["r"].max() <= 5
        if c["regime"] in "ab":
            assert c["cands"].shape == (c["U"], min(30, c["I"])) and c["rank_ref"].shape == (c["U"], min(TOPK, c["I"], 30))
            assert all(len(set(row)) == len(row) for row in c["cands"].tolist())
        if c["regime"] == "a":
            assert c["oracle_dev"] == 0.0 and c["decided"][c["has"]].all()
    assert os.path.getsize(os.path.join(GOLDEN, "kat_knn.npz")) < (1 << 20)


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_reproduces_the_reference_W(tag):
    check_W(case(tag), oracle_W(tag))


@pytest.mark.parametrize("tag", SCORED)
def test_oracle_scores_and_lists(tag):
    c = case(tag)
    full = O.pred(c["X"], oracle_W(tag), c["model"])
    sc = np.take_along_axis(full, c["cands"], 1)
    check_scores(c, sc, O.rank_lists(sc, c["cands"], TOPK))
    assert np.array_equal(O.decided(c["scores_ref"], c["tol"].max()), c["decided"])
    assert np.array_equal(O.rank_lists(c["scores_ref"], c["cands"], TOPK), c["rank_ref"])


def test_select_tie_rule_and_zeros():
    Wr = np.array([[0, 2, 2, 2, 1, 0], [-1, 0, -0.0, -2, -3, -4], [0, 0, 0, 0, 0, 0]], dtype=np.float32)
    cnt, rows, vals = O.select(Wr, 2)
    assert cnt.tolist() == [2, 0, 0] and rows[0].tolist() == [1, 2] and vals[0].tolist() == [2, 2]
    assert rows[1].tolist() == [-1, -1] and not vals[1].any()              # the zeros outrank the negatives and are dropped
    cnt, rows, vals = O.select(Wr, 4)
    assert cnt.tolist() == [4, 2, 0] and rows[0].tolist() == [1, 2, 3, 4] and rows[1].tolist() == [0, 3, -1, -1]
    cnt, rows, _ = O.select(Wr, 9)                                          # K above n
    assert cnt.tolist() == [4, 4, 0] and rows.shape == (3, 9) and rows[1, :5].tolist() == [0, 3, 4, 5, -1]
