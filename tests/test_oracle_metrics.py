"""tests/metrics_oracle.py against the reference's stored values (tests/golden/kat_metrics.npz, written by
tests/golden/make_golden_metrics.py from the real daisy.utils.metrics and daisy.model.PopRecommender): the regimes of the
oracle's docstring, and that the fixtures hold the cases they are meant to hold."""
import os

import numpy as np
import pytest

import metrics_oracle as O

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_metrics.npz"))


def golden(tag):
    fx = O.FIXTURES[tag]
    per = {m: GOLD[f"{tag}_per_{m}"] for m in O.fixture_metrics(fx) if m != "coverage"}
    means = {m: GOLD[f"{tag}_mean_{m}"] for m in O.fixture_metrics(fx)}
    return per, means, GOLD[f"{tag}_cover"]


@pytest.mark.parametrize("tag", list(O.FIXTURES))
def test_oracle_meets_the_regimes_against_the_reference(tag):
    fx, data = O.FIXTURES[tag], O.make_fixture(tag)
    pred = data["pred"]
    assert np.array_equal(GOLD[f"{tag}_pred_sum"], [pred.sum(), (pred * np.arange(1, fx["K"] + 1)).sum()]), \
        "the fixture no longer comes out of its seed as it did when the golden file was written"
    per, means, cover = O.kpis(pred, data["test_ur"], data["test_u"], fx["cutoffs"], O.fixture_metrics(fx), fx["item_num"],
                               data["item_pop"], data["i_categories"])
    ref_per, ref_means, ref_cover = golden(tag)
    O.check_regimes(per, means, ref_per, ref_means, fx["cutoffs"], fx["int_pop"], what=f"{tag}: ")
    assert np.array_equal(cover, ref_cover)
    assert np.array_equal(cover / fx["item_num"], ref_means["coverage"])


def test_fixtures_hold_their_edge_cases():
    data, fx = O.make_fixture("k50"), O.FIXTURES["k50"]
    ref_per, _, _ = golden("k50")
    last = len(fx["cutoffs"]) - 1
    pre = ref_per["precision"][last]
    assert pre[1] == 0.0 and np.isnan(ref_per["auc"][last][1]) and np.isnan(ref_per["f1"][last][1])        # no hit
    assert pre[2] == 1.0 and np.isnan(ref_per["auc"][last][2]) and not np.isnan(ref_per["f1"][last][2])    # only hits
    assert data["pred"][3, 0] == data["pred"][3, -1] and data["pred"][3, 0] in data["test_ur"][data["test_u"][3]]
    assert len(set(data["test_u"])) < len(data["test_u"]) and data["test_u"] != sorted(data["test_u"])
    assert data["pred"].min() == 0 and data["pred"].max() == fx["item_num"] - 1
    assert np.isnan(golden("k1")[0]["diversity"][0]).all()                                                # k = 1: no pair
    # a duplicate hit counts once for popularity and per position for precision
    one = {0: {7}}
    per, _, _ = O.kpis(np.array([[7, 3, 7]]), one, [0], [3], ["precision", "popularity"], 10, np.arange(10.0))
    assert per["precision"][0, 0] == 2 / 3 and per["popularity"][0, 0] == 7.0


@pytest.mark.parametrize("tag", list(O.POP_FIXTURES))
def test_pop_oracle_equals_the_reference(tag):
    fx, data = O.POP_FIXTURES[tag], O.make_pop_fixture(tag)
    cnt, score = O.pop_fit(data["items"], fx["item_num"])
    assert np.array_equal(cnt, GOLD[f"pop_{tag}_cnt"]) and np.array_equal(score, GOLD[f"pop_{tag}_score"])
    mine, ref = O.pop_rank(score, data["cands"], fx["topk"]), GOLD[f"pop_{tag}_rank"].astype(np.int64)
    assert np.array_equal(score[mine], score[ref])
    if tag == "distinct":
        assert np.unique(cnt).size == cnt.size and np.array_equal(mine, ref)
    if tag == "ties":
        assert (cnt == 0).sum() > fx["item_num"] // 2
