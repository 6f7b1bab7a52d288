#!/usr/bin/env python
"""Golden values for the ranking KPIs and MostPop, generated from the REAL reference (`daisy.utils.metrics` and
`daisy.model.PopRecommender`, imported from the reference checkout; nothing is copied).  Runs only where the reference
exists; the output is committed:

    python tests/golden/make_golden_metrics.py            # -> tests/golden/kat_metrics.npz
    python tests/golden/make_golden_metrics.py --time     # only prints the reference's seconds per user on this host

Per fixture of tests/metrics_oracle.py::FIXTURES (`<tag>_*`; the inputs are rebuilt from the fixture's seed, a checksum of
the lists is stored): the reference's per-list values (each reference function called on one-list slices), its means from
the full call, its coverage, and for CALC_FIXTURES the DataFrame of `calc_ranking_results`.  Before anything is written the
script ASSERTS that the oracle meets the regimes of metrics_oracle.py's docstring against these values: if that fails, a
bound's derivation is wrong - do not change a seed.

Per fixture of POP_FIXTURES (`pop_<tag>_*`): the reference's `item_cnt_ref`, `item_score`, `rank` lists and `full_rank`.
"""
import logging
import os
import sys
import tempfile
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402  (puts the reference checkout and the logging shims on sys.path; shims np.asfarray)

import pandas as pd  # noqa: E402
import torch  # noqa: E402

import daisy.utils.metrics as RM  # noqa: E402
from daisy.model.PopRecommender import MostPop  # noqa: E402

import metrics_oracle as O  # noqa: E402

warnings.filterwarnings("ignore", category=RuntimeWarning)      # the reference's 0 / 0 (f1, auc) and mean of nothing

REF_FN = {"precision": RM.Precision, "recall": RM.Recall, "hit": RM.HR, "mrr": RM.MRR, "map": RM.MAP, "ndcg": RM.NDCG,
          "f1": RM.F1, "auc": RM.AUC}


def reference_values(fixture, cutoffs, metrics, item_num):
    """-> (per {name: [nc, n]}, means {name: [nc]}) from the reference's own functions"""
    test_ur, test_u, pred = fixture["test_ur"], fixture["test_u"], fixture["pred"]
    n = pred.shape[0]
    per = {m: np.zeros((len(cutoffs), n)) for m in metrics if m != "coverage"}
    means = {m: np.zeros(len(cutoffs)) for m in metrics}
    for c, k in enumerate(cutoffs):
        top = pred[:, :k]
        for m in metrics:
            if m == "coverage":
                means[m][c] = RM.Coverage(top, item_num)
                continue
            if m == "popularity":
                one = lambda s, us: RM.Popularity(test_ur, s, us, fixture["item_pop"])         # noqa: E731
            elif m == "diversity":
                one = lambda s, us: RM.Diversity(s, fixture["i_categories"])                   # noqa: E731
            else:
                one = lambda s, us, f=REF_FN[m]: f(test_ur, s, us)                             # noqa: E731
            for idx in range(n):
                per[m][c, idx] = one(top[idx:idx + 1], test_u[idx:idx + 1])
            means[m][c] = one(top, test_u)
    return per, means


def calc_frame(fixture, topk, item_num, tmp):
    cfg = {"logger": logging.getLogger("golden"), "res_path": tmp, "metrics": O.CALC_KPIS, "item_num": item_num,
           "item_pop": fixture["item_pop"], "i_categories": fixture["i_categories"], "topk": topk}
    return RM.calc_ranking_results(fixture["test_ur"], fixture["pred"], fixture["test_u"], cfg)


def pop_reference(tag):
    fx, data = O.POP_FIXTURES[tag], O.make_pop_fixture(tag)
    cfg = G.base_config(item_num=fx["item_num"], topk=fx["topk"], IID_NAME="item", gpu="0")
    m = MostPop(cfg)
    m.device = "cpu"
    m.fit(pd.DataFrame({"item": data["items"]}))
    loader = [(torch.from_numpy(data["us"]), torch.from_numpy(data["cands"]))]
    return dict(cnt=m.item_cnt_ref.copy(), score=m.item_score.copy(), rank=m.rank(loader),
                full=np.asarray(m.full_rank(0)).astype(np.int64))


def time_reference():
    rng = np.random.default_rng(0)
    n, K, I = 500, 50, 1682
    test_ur = {u: set(int(x) for x in rng.choice(I, 10, replace=False)) for u in range(n)}
    pred = rng.integers(0, I, (n, K))
    cfg = {"logger": logging.getLogger("golden"), "res_path": tempfile.gettempdir(), "metrics": O.DEFAULT_KPIS, "item_num": I,
           "item_pop": None, "i_categories": None, "topk": K}
    t0 = time.perf_counter()
    RM.calc_ranking_results(test_ur, pred, list(range(n)), cfg)
    t1 = time.perf_counter()
    cats = (rng.random((I, 19)) < 0.3).astype(np.int64)
    RM.Diversity(pred[:50], cats)
    t2 = time.perf_counter()
    print(f"reference calc_ranking_results, default five KPIs, six cutoffs, top-50, 1682 items: {(t1 - t0) / n * 1e3:.2f} ms "
          f"per user ({n} users)")
    print(f"reference Diversity, K = 50, 19 categories: {(t2 - t1) / 50 * 1e3:.2f} ms per user (50 users)")


def main():
    if "--time" in sys.argv:
        return time_reference()
    out = {}
    for tag, fx in O.FIXTURES.items():
        data = O.make_fixture(tag)
        metrics, cutoffs, I = O.fixture_metrics(fx), fx["cutoffs"], fx["item_num"]
        t0 = time.perf_counter()
        ref_per, ref_means = reference_values(data, cutoffs, metrics, I)
        o_per, o_means, o_cover = O.kpis(data["pred"], data["test_ur"], data["test_u"], cutoffs, metrics, I,
                                         data["item_pop"], data["i_categories"])
        O.check_regimes(o_per, o_means, ref_per, ref_means, cutoffs, fx["int_pop"], what=f"{tag}: oracle vs reference, ")
        assert np.array_equal(o_cover / I, ref_means["coverage"]), tag
        out[f"{tag}_pred_sum"] = np.array([data["pred"].sum(), (data["pred"] * np.arange(1, fx["K"] + 1)).sum()])
        for m, v in ref_per.items():
            out[f"{tag}_per_{m}"] = v
        for m, v in ref_means.items():
            out[f"{tag}_mean_{m}"] = v
        out[f"{tag}_cover"] = o_cover
        line = f"{tag}: n={fx['n']} K={fx['K']} item_num={I}: oracle within the regimes of the reference"
        if tag in O.CALC_FIXTURES:
            frame = calc_frame(data, fx["K"], I, os.path.join(tempfile.mkdtemp(), "res"))
            assert list(frame.columns) == ["KPI@K"] + cutoffs, frame.columns
            assert list(frame["KPI@K"]) == [RM.metrics_name_config[m] for m in O.CALC_KPIS]
            vals = frame[cutoffs].to_numpy(dtype=np.float64)
            for row, m in enumerate(O.CALC_KPIS):
                assert np.array_equal(vals[row], ref_means[m], equal_nan=True), (tag, m)
            out[f"{tag}_frame"] = vals
            line += "; calc_ranking_results stored"
        print(line, f"({time.perf_counter() - t0:.1f} s)")
    for tag in O.POP_FIXTURES:
        ref = pop_reference(tag)
        data, fx = O.make_pop_fixture(tag), O.POP_FIXTURES[tag]
        cnt, score = O.pop_fit(data["items"], fx["item_num"])
        assert np.array_equal(cnt, ref["cnt"]) and np.array_equal(score, ref["score"]), tag
        mine = O.pop_rank(score, data["cands"], fx["topk"])
        assert np.array_equal(score[mine], score[ref["rank"].astype(np.int64)]), tag
        if tag == "distinct":
            assert np.array_equal(mine, ref["rank"].astype(np.int64)), tag
            assert np.array_equal(np.argsort(-score, kind="stable")[:fx["topk"]], ref["full"]), tag
            assert np.unique(cnt).size == cnt.size
        for k, v in ref.items():
            out[f"pop_{tag}_{k}"] = v
        print(f"pop {tag}: counts and scores bitwise, ranked scores equal")
    path = os.path.join(HERE, "kat_metrics.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
