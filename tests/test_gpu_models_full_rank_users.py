"""full_rank_users of EASE, SLiM, ItemKNNCF, UserKNNCF and PureSVD on a small fitted model: against
tests/rank_f64_oracle.py applied to the model's own all-item scores, against the model's full_rank, and through the KPI
frame.  Every test here fails without the feature (NotImplementedError from the base class)."""
import functools
import logging

import numpy as np
import pandas as pd
import pytest
import torch

import rank_f64_oracle as RO
from conftest import mf_config

pytestmark = pytest.mark.gpu
NAMES = ("ease", "slim", "itemknn", "userknn", "puresvd")
U, I, TOPK = 60, 90, 10


def _build(name, topk=TOPK):
    from daisyrec_amd import model as M
    base = dict(user_num=U, item_num=I, topk=topk)
    if name == "ease":
        return M.EASE(mf_config(algo_name="ease", reg=50.0, **base))
    if name == "slim":
        return M.SLiM(mf_config(algo_name="slim", alpha=0.05, elastic=0.1, **base))
    if name == "puresvd":
        return M.PureSVD(mf_config(algo_name="puresvd", factors=8, **base))
    cls = M.ItemKNNCF if name == "itemknn" else M.UserKNNCF
    return cls(mf_config(algo_name=name, maxk=15, shrink=10, normalize=True, similarity="cosine", **base))


@functools.lru_cache(maxsize=None)
def _frame():
    """about 60 x 90, ratings 1..5, every user with at least one item; (train frame, train_ur, test_ur)"""
    rng = np.random.default_rng(31)
    seen = rng.random((U, I)) < 0.18
    seen[np.arange(U), rng.integers(0, I, U)] = True
    u, i = np.nonzero(seen)
    test = rng.random(u.size) < 0.2
    test[np.unique(u, return_index=True)[1]] = False            # the first item of every user trains
    r = rng.integers(1, 6, u.size).astype(np.float64)
    df = pd.DataFrame({"user": u[~test], "item": i[~test], "rating": r[~test]})
    train_ur = {int(a): set(i[~test][u[~test] == a].tolist()) for a in range(U)}
    test_ur = {int(a): set(i[test][u[test] == a].tolist()) for a in np.unique(u[test])}
    assert all(train_ur[a] for a in range(U))
    return df, train_ur, test_ur


@functools.lru_cache(maxsize=None)
def _fitted(name):
    m = _build(name)
    df = _frame()[0]
    if name == "slim":
        m.fit(df, verbose=False)
    else:
        m.fit(df)
    return m


def _all_scores(name, m, users):
    """the model's own all-item scores [n, I]: the existing kernels"""
    if name == "slim":
        return m._scores(users).cpu().numpy()
    return m._rank(users, None, 0)[0].cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_equals_the_oracle_on_the_models_own_scores(name, tmp_path):
    from daisyrec_amd.utils.metrics import calc_ranking_results
    from daisyrec_amd.utils.utils import user_csr
    m = _fitted(name)
    _, train_ur, test_ur = _frame()
    test_u = list(test_ur)[::-1] + [list(test_ur)[0]]           # unsorted, one user twice
    scores = _all_scores(name, m, test_u)
    assert scores.shape == (len(test_u), I) and scores.dtype == (np.float32 if name == "slim" else np.float64)
    want_ids, want_sc = RO.rank_lists(scores, TOPK, users=test_u, exclude=train_ur)
    preds = m.full_rank_users(test_u, exclude=train_ur)
    assert isinstance(preds, torch.Tensor) and preds.is_cuda and preds.dtype == torch.int64 and preds.shape == (len(test_u), TOPK)
    assert np.array_equal(preds.cpu().numpy(), want_ids)
    pairs = np.array([(a, b) for a in range(U) for b in sorted(train_ur[a])], np.int64)
    ids, sc = m.full_rank_users(np.asarray(test_u), exclude=user_csr(pairs.T, U), return_scores=True)
    assert torch.equal(ids, preds)                              # dict and device CSR: the same exclusion
    sc = sc.cpu().numpy()
    assert sc.dtype == want_sc.dtype and np.array_equal(sc.view(np.uint8), want_sc.view(np.uint8))
    assert not any(set(row.tolist()) & train_ur[a] for row, a in zip(want_ids, test_u))
    # the lists feed the KPI frame
    cfg = {"logger": logging.getLogger("full-rank-f64-test"), "res_path": str(tmp_path / "res"), "item_num": I, "topk": TOPK,
           "metrics": ["recall", "mrr", "ndcg", "hit", "precision"]}
    users = list(test_ur)
    got = calc_ranking_results(test_ur, m.full_rank_users(users, exclude=train_ur), users, cfg)
    ref = calc_ranking_results(test_ur, RO.rank_lists(_all_scores(name, m, users), TOPK, users=users, exclude=train_ur)[0],
                               users, cfg)
    assert got.equals(ref)


@pytest.mark.parametrize("name", NAMES)
def test_rows_equal_full_rank_without_exclusion(name):
    m = _fitted(name)
    users = [5, 0, 59, 5, 17, 33]
    got = m.full_rank_users(users).cpu().numpy()
    assert got.shape == (len(users), TOPK)
    for b, u in enumerate(users):
        assert np.array_equal(got[b], m.full_rank(u)), (name, u)
    assert torch.equal(m.full_rank_users(torch.tensor(users), exclude=None), m.full_rank_users(np.asarray(users)))


@pytest.mark.parametrize("name", NAMES)
def test_short_lists_errors_and_the_unfitted_model(name, tmp_path):
    from daisyrec_amd.utils.metrics import calc_ranking_results
    m = _fitted(name)
    few = m.full_rank_users([2], exclude={2: set(range(I - 3))}).cpu().numpy()
    assert sorted(few[0, :3].tolist()) == [I - 3, I - 2, I - 1] and np.all(few[0, 3:] == -1)
    cfg = {"logger": logging.getLogger("full-rank-f64-test"), "res_path": str(tmp_path / "res"), "item_num": I, "topk": TOPK,
           "metrics": ["recall", "hit"]}
    with pytest.raises(ValueError, match="pred_ur: item id -1"):
        calc_ranking_results({2: {I - 1}}, few, [2], cfg)
    with pytest.raises(IndexError):
        m.full_rank_users([0, U])
    indptr = np.zeros(U + 1, np.int64)
    indptr[2:] = 2
    with pytest.raises(ValueError, match="ascending"):
        m.full_rank_users([1], exclude=(torch.from_numpy(indptr).cuda(), torch.tensor([9, 3], dtype=torch.int32).cuda()))
    with pytest.raises(RuntimeError, match="fit"):
        _build(name).full_rank_users([1])
    m.topk = 129                                                # (the cutoff of a call, read when it is made)
    try:
        with pytest.raises(ValueError, match="cap of 128"):
            m.full_rank_users([1])
    finally:
        m.topk = TOPK
    # what does not change: the base class and MostPop
    from daisyrec_amd import model as M
    with pytest.raises(NotImplementedError, match="full_rank_users"):
        M.AbstractRecommender().full_rank_users([1])
    other = M.MostPop(mf_config(user_num=U, item_num=I, topk=10, algo_name="mostpop"))
    with pytest.raises(NotImplementedError, match="full_rank_users"):
        other.full_rank_users([1])
