"""ops.full_rank_users / model.full_rank_users (csrc/rank_full.hip) against tests/full_rank_oracle.py:
bit for bit on exact tables, by the derived fp32 conditions on real-valued ones."""
import logging

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import full_rank_oracle as FO
from conftest import mf_config

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _tables(rng, U, I, d, lo=-128, hi=128, scale=1.0):
    P = (rng.integers(lo, hi + 1, size=(U, d)) * scale).astype(np.float32)
    Q = (rng.integers(lo, hi + 1, size=(I, d)) * scale).astype(np.float32)
    return P, Q


def _csr(rows, U):
    """(indptr int64 [U + 1], items int32) of {user: list of items}, the lists as given"""
    indptr = np.zeros(U + 1, np.int64)
    for u in range(U):
        indptr[u + 1] = indptr[u] + len(rows.get(u, ()))
    items = np.array([i for u in range(U) for i in rows.get(u, ())], np.int32)
    return indptr, items


def _random_rows(rng, U, I, share=0.15):
    return {u: sorted(rng.choice(I, size=int(rng.integers(0, max(1, int(I * share)) + 1)), replace=False).tolist())
            for u in range(U)}


def _run(P, Q, users, topk, exclude=None, biases=None, slices=0, validate=True):
    from daisyrec_amd import ops
    ex = None if exclude is None else tuple(_t(x) for x in exclude)
    b = None if biases is None else tuple(_t(np.asarray(x, np.float32)) for x in biases)
    ids, scores = ops.full_rank_users(_t(P), _t(Q), _t(np.asarray(users, np.int64)), topk, exclude=ex, biases=b,
                                      return_scores=True, item_slices=slices, validate=validate)
    assert ids.is_cuda and ids.dtype == torch.int64 and scores.dtype == torch.float32
    return ids.cpu().numpy(), scores.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _assert_exact(P, Q, users, topk, exclude=None, biases=None, slices=0, scale=1.0, validate=True, what=""):
    ids, scores = _run(P, Q, users, topk, exclude, biases, slices, validate)
    rows = None
    if exclude is not None:                 # (an entry >= I excludes nothing)
        rows = {int(u): set(int(i) for i in exclude[1][exclude[0][u]:exclude[0][u + 1]] if 0 <= i < Q.shape[0])
                for u in set(np.asarray(users).tolist())}
    want_ids, want_scores = FO.full_rank_exact(P, Q, np.asarray(users), topk, exclude=rows, biases=biases, scale=scale)
    assert np.array_equal(ids, want_ids), (what, np.argwhere(ids != want_ids)[:5])
    assert _same_bits(scores, want_scores), what
    return ids, scores


# d: k tails against the 16-deep tile, rows that are no 16-byte multiples, the largest d; I and n: below, at and above
# one 128-item / 64-user tile; topk up to the cap and above I; slices: auto, one, several, more than there are tiles
GRID = [(1, 1, 1, 1, 0), (3, 31, 63, 10, 1), (16, 128, 64, 50, 2), (50, 129, 65, 128, 3), (64, 333, 130, 10, 7),
        (100, 333, 64, 50, 1000), (130, 129, 130, 128, 2), (512, 333, 65, 50, 0), (64, 31, 1, 50, 0),
        (16, 333, 130, 128, 3), (3, 128, 63, 1, 7), (512, 1, 64, 10, 1000), (130, 31, 65, 10, 3), (50, 333, 1, 128, 7),
        (100, 128, 130, 1, 2), (1, 129, 63, 50, 1000)]


@pytest.mark.parametrize("case", range(len(GRID)))
def test_exact_grid(case):
    d, I, n, topk, slices = GRID[case]
    rng = np.random.default_rng(100 + case)
    U = 97
    scale = 1.0 if case % 2 == 0 else 2.0 ** -3
    P, Q = _tables(rng, U, I, d, scale=scale)
    users = rng.integers(0, U, size=n)                  # unsorted; duplicates as soon as n is not tiny
    if n >= 3:
        users[-1] = users[0]
    exclude = _csr(_random_rows(rng, U, I), U) if case % 3 else None
    _assert_exact(P, Q, users, topk, exclude=exclude, slices=slices, scale=scale, what=GRID[case])


@pytest.mark.parametrize("slices", [1, 3])
def test_ties_go_to_the_lower_id(slices):
    rng = np.random.default_rng(5)
    U, I, d = 70, 333, 16
    P, Q = _tables(rng, U, I, d, lo=-2, hi=2)
    s = P.astype(np.int64) @ Q.astype(np.int64).T
    top = -np.sort(-s, axis=1)[:, :11]
    assert np.all((top[:, 1:] == top[:, :-1]).any(axis=1))         # every user has a tie inside the top 11
    _assert_exact(P, Q, np.arange(U), 11, slices=slices)
    _assert_exact(P, Q, np.arange(U), 128, exclude=_csr(_random_rows(rng, U, I), U), slices=slices)


@pytest.mark.parametrize("slices", [0, 1, 3])
def test_all_zero_tables_give_the_lowest_eligible_ids(slices):
    U, I, d, topk = 70, 333, 16, 50
    P, Q = np.zeros((U, d), np.float32), np.zeros((I, d), np.float32)
    ids, scores = _run(P, Q, np.arange(U), topk, slices=slices)
    assert np.array_equal(ids, np.tile(np.arange(topk), (U, 1))) and not scores.any()
    rows = {u: list(range(u, 140 + u)) for u in range(U)}           # across the tile boundary at 128
    ids, _ = _run(P, Q, np.arange(U), topk, exclude=_csr(rows, U), slices=slices)
    for u in range(U):
        want = [j for j in range(I) if not u <= j < 140 + u][:topk]
        assert ids[u].tolist() == want, u


@pytest.mark.parametrize("slices", [0, 2, 3])
def test_exclusion_rows(slices):
    rng = np.random.default_rng(11)
    U, I, d, topk = 12, 333, 16, 10
    P, Q = _tables(rng, U, I, d)
    rows = {1: list(range(I)),                              # everything: all -1
            2: [j for j in range(I) if j % 70 != 3],        # leaves 5 items: fewer than topk
            3: [0, 127, 128, 129, I - 1],                   # the tile edges
            4: [5, 5, 5, 200, 200]}                         # duplicated entries
    users = [3, 0, 1, 2, 4, 3, 4, 11]                       # user 0 and 11: empty rows; 3 and 4 twice
    ids, scores = _assert_exact(P, Q, users, topk, exclude=_csr(rows, U), slices=slices)
    assert np.all(ids[2] == -1) and np.all(np.isneginf(scores[2]))
    assert np.all(ids[3, :5] >= 0) and np.all(ids[3, 5:] == -1)
    assert np.array_equal(ids[0], ids[5]) and np.array_equal(ids[4], ids[6])
    none, _ = _assert_exact(P, Q, users, topk, exclude=None, slices=slices)
    assert np.array_equal(none[1], ids[1]) and np.array_equal(none[7], ids[7])       # empty rows: nothing excluded


def test_an_entry_beyond_the_items_is_harmless_without_validation():
    """row contents are only compared, never used as an index: ids >= I exclude nothing and touch nothing"""
    rng = np.random.default_rng(12)
    U, I, d = 6, 200, 16
    P, Q = _tables(rng, U, I, d)
    rows = {0: [7, 199, 200, 400, 100000, 2 ** 31 - 1], 3: [2 ** 31 - 1] * 9, 5: [0, 128, 1 << 20]}
    for slices in (1, 2):
        _assert_exact(P, Q, [0, 3, 5, 1], 20, exclude=_csr(rows, U), slices=slices, validate=False)


def test_fm_biases_exact():
    rng = np.random.default_rng(13)
    U, I, d = 50, 333, 20
    P, Q = _tables(rng, U, I, d)
    biases = (rng.integers(-999, 1000, size=U).astype(np.float32), rng.integers(-999, 1000, size=I).astype(np.float32),
              np.array([-41.0], np.float32))
    users = rng.permutation(U)
    for slices in (0, 2):
        ids, _ = _assert_exact(P, Q, users, 50, biases=biases, exclude=_csr(_random_rows(rng, U, I), U), slices=slices)
    plain, _ = _run(P, Q, users, 50)
    assert not np.array_equal(plain, _run(P, Q, users, 50, biases=biases)[0])


def test_nan_ranks_first_then_inf():
    rng = np.random.default_rng(14)
    U, I, d, topk = 40, 300, 16, 10
    P = rng.integers(1, 129, size=(U, d)).astype(np.float32)
    Q = rng.integers(-128, 129, size=(I, d)).astype(np.float32)
    Qs = Q.copy()
    Qs[217] = np.nan                                        # every score of item 217 is NaN
    Qs[5] = 0.0
    Qs[5, 0] = np.inf                                       # P > 0: every score of item 5 is +inf
    rest, rest_scores = FO.full_rank_exact(P, Q, np.arange(U), topk - 2, exclude={u: {5, 217} for u in range(U)})
    for slices in (1, 3):
        ids, scores = _run(P, Qs, np.arange(U), topk, slices=slices)
        assert np.all(ids[:, 0] == 217) and np.all(np.isnan(scores[:, 0]))
        assert np.all(ids[:, 1] == 5) and np.all(np.isposinf(scores[:, 1]))
        assert np.array_equal(ids[:, 2:], rest) and _same_bits(scores[:, 2:], rest_scores)


@pytest.fixture(scope="module")
def real_tables():
    rng = np.random.default_rng(2022)
    U, I, d = 300, 1500, 64
    P = rng.normal(0, 0.1, (U, d)).astype(np.float32)
    Q = rng.normal(0, 0.1, (I, d)).astype(np.float32)
    biases = (rng.normal(0, 0.05, U).astype(np.float32), rng.normal(0, 0.05, I).astype(np.float32),
              np.array([-0.2], np.float32))
    exclude = _csr(_random_rows(rng, U, I, share=0.1), U)
    return P, Q, biases, exclude


@pytest.mark.parametrize("with_excl,with_bias", [(False, False), (True, False), (False, True), (True, True)])
def test_toleranced_form(real_tables, with_excl, with_bias):
    P, Q, biases, exclude = real_tables
    users = np.arange(P.shape[0])
    ids, scores = _run(P, Q, users, 50, exclude=exclude if with_excl else None, biases=biases if with_bias else None)
    FO.check_toleranced(P, Q, users, 50, ids, scores, exclude=exclude if with_excl else None,
                        biases=biases if with_bias else None)


def test_bitwise_equal_between_runs_and_slice_counts(real_tables):
    P, Q, biases, exclude = real_tables
    users = np.arange(P.shape[0])[::-1].copy()
    first = _run(P, Q, users, 50, exclude=exclude, biases=biases, slices=0)
    for slices in (0, 1, 2, 3, 7, 1000):
        ids, scores = _run(P, Q, users, 50, exclude=exclude, biases=biases, slices=slices)
        assert np.array_equal(ids, first[0]) and _same_bits(scores, first[1]), slices


def test_validation_and_the_cap():
    from daisyrec_amd import ops
    rng = np.random.default_rng(15)
    U, I, d = 9, 200, 16
    P, Q = (_t(x) for x in _tables(rng, U, I, d))
    for bad in ([0, 9], [-1, 2]):
        with pytest.raises(IndexError, match="out of bounds"):
            ops.full_rank_users(P, Q, torch.tensor(bad), 5)
    good = _csr({2: [1, 5, 5, 9]}, U)
    assert ops.full_rank_users(P, Q, torch.tensor([2]), 5, exclude=tuple(_t(x) for x in good)).shape == (1, 5)
    unsorted = _csr({2: [5, 1], 3: [0]}, U)
    with pytest.raises(ValueError, match="ascending"):
        ops.full_rank_users(P, Q, torch.tensor([2]), 5, exclude=tuple(_t(x) for x in unsorted))
    out = ops.full_rank_users(P, Q, torch.tensor([2]), 5, exclude=tuple(_t(x) for x in unsorted), validate=False)
    assert out.shape == (1, 5) and bool(((out >= 0) & (out < I)).all())        # harmless: at most a missed exclusion
    short = (_t(good[0][:-1]), _t(good[1]))
    with pytest.raises(ValueError, match="indptr"):
        ops.full_rank_users(P, Q, torch.tensor([2]), 5, exclude=short)
    with pytest.raises(ValueError, match="cap of 128"):
        ops.full_rank_users(P, Q, torch.tensor([2]), 129)
    assert ops.full_rank_users(P, Q, torch.tensor([2]), 128).shape == (1, 128)
    assert ops.full_rank_users(P, Q, torch.tensor([2]), 5, return_scores=False).dtype == torch.int64
    empty = ops.full_rank_users(P, Q, torch.zeros(0, dtype=torch.int64), 5)
    assert empty.shape == (0, 5)


# ---- model level ---------------------------------------------------------------------------------------------------------
def _frame(U, I, rng, n_train=500, n_test=80):
    tr = np.unique(np.stack([rng.integers(0, U, n_train), rng.integers(0, I, n_train)], 1), axis=0)
    train_ur, test_ur = {}, {}
    for u, i in tr:
        train_ur.setdefault(int(u), set()).add(int(i))
    for u, i in zip(rng.integers(0, U, n_test), rng.integers(0, I, n_test)):
        if int(i) not in train_ur.get(int(u), ()):
            test_ur.setdefault(int(u), set()).add(int(i))
    return tr, train_ur, test_ur


def _model(name, U, I, tr, train_ur, topk):
    from daisyrec_amd import model as M
    from daisyrec_amd.model.Item2VecRecommender import Item2Vec
    from daisyrec_amd.model.LightGCNRecommender import LightGCN
    inter = sp.coo_matrix((np.ones(len(tr), np.float32), (tr[:, 0], tr[:, 1])), shape=(U, I))
    torch.manual_seed(7)
    if name == "mf":            # factors = 50: the automatic row pitch pads the tables to 64 columns
        m = M.MF(mf_config(user_num=U, item_num=I, factors=50, topk=topk))
        assert m._tables()[0].shape[1] == 64
    elif name == "fm":
        m = M.FM(mf_config(user_num=U, item_num=I, factors=24, topk=topk))
        torch.nn.init.normal_(m.u_bias.weight, std=0.01)
        torch.nn.init.normal_(m.i_bias.weight, std=0.01)
        m.bias_.data.fill_(0.3)
    elif name == "lightgcn":
        m = LightGCN(mf_config(user_num=U, item_num=I, factors=16, num_layers=2, algo_name="lightgcn", reg_1=0.0, reg_2=0.0,
                               inter_matrix=inter, topk=topk))
    elif name == "ngcf":
        m = M.NGCF(mf_config(user_num=U, item_num=I, factors=16, algo_name="ngcf", hidden_size_list=[16, 8], node_dropout=0.0,
                             mess_dropout=0.0, reg_1=0.0, reg_2=0.0, inter_matrix=inter, topk=topk))
    else:
        m = Item2Vec(mf_config(user_num=U, item_num=I, factors=20, train_ur=train_ur, topk=topk, algo_name="item2vec"))
    return m


def _model_tables(name, m):
    if name in ("mf", "fm"):
        P, Q = m._tables()
        d = m.embed_user.weight.shape[1]
        assert not P[:, d:].any()
        b = m._biases()
        return P[:, :d].cpu().numpy(), Q[:, :d].cpu().numpy(), None if b is None else tuple(x.cpu().numpy() for x in b)
    if name in ("lightgcn", "ngcf"):
        ue, ie = m._restore()
        return ue.cpu().numpy(), ie.cpu().numpy(), None
    Uemb, S = m._tables()
    return Uemb.cpu().numpy(), S.cpu().numpy(), None


@pytest.mark.parametrize("name", ["mf", "fm", "lightgcn", "ngcf", "item2vec"])
def test_model_full_rank_users_feeds_the_kpi_frame(name, tmp_path):
    from daisyrec_amd.utils.metrics import calc_ranking_results
    from daisyrec_amd.utils.utils import user_csr
    rng = np.random.default_rng(21)
    U, I, topk = 70, 150, 10
    tr, train_ur, test_ur = _frame(U, I, rng)
    m = _model(name, U, I, tr, train_ur, topk)
    m.eval()
    test_u = list(test_ur)
    preds = m.full_rank_users(test_u, exclude=train_ur)
    assert isinstance(preds, torch.Tensor) and preds.is_cuda and preds.dtype == torch.int64 and preds.shape == (len(test_u), topk)
    P, Q, biases = _model_tables(name, m)
    s = P.astype(np.float64)[test_u] @ Q.astype(np.float64).T
    if biases is not None:
        s = s + ((biases[0].reshape(-1).astype(np.float64)[test_u][:, None] + biases[1].reshape(-1).astype(np.float64)[None, :])
                 + float(biases[2].reshape(-1)[0]))
    want, _ = FO.rank_lists(s, FO.exclusion_sets(train_ur, test_u), topk)
    ids, scores = m.full_rank_users(np.asarray(test_u), exclude=user_csr(tr.T, U), return_scores=True)
    assert torch.equal(ids, preds)                          # dict and device CSR: the same exclusion
    FO.check_toleranced(P, Q, test_u, topk, ids.cpu().numpy(), scores.cpu().numpy(), exclude=train_ur, biases=biases)
    cfg = {"logger": logging.getLogger("full-rank-test"), "res_path": str(tmp_path / "res"), "item_num": I, "topk": topk,
           "metrics": ["recall", "mrr", "ndcg", "hit", "precision"]}
    got = calc_ranking_results(test_ur, preds, test_u, cfg)
    ref = calc_ranking_results(test_ur, want, test_u, cfg)
    assert got.equals(ref)
    assert torch.equal(m.full_rank_users(torch.tensor(test_u), exclude=None), m.full_rank_users(test_u))


def test_rows_equal_full_rank_of_the_existing_path():
    """exact tables, no exclusion: every row is model.full_rank(u) - the tie rule is the same, lower id first"""
    from daisyrec_amd import model as M
    rng = np.random.default_rng(22)
    U, I, d, topk = 24, 333, 16, 50
    P, Q = _tables(rng, U, I, d, lo=-3, hi=3)                # many ties
    m = M.MF(mf_config(user_num=U, item_num=I, factors=d, topk=topk))
    with torch.no_grad():
        m.embed_user.weight.copy_(torch.from_numpy(P))
        m.embed_item.weight.copy_(torch.from_numpy(Q))
    got = m.full_rank_users(list(range(U))).cpu().numpy()
    for u in range(U):
        assert np.array_equal(got[u], m.full_rank(u)), u
    assert np.array_equal(got, FO.full_rank_exact(P, Q, np.arange(U), topk)[0])


def test_model_errors(tmp_path):
    from daisyrec_amd import model as M
    from daisyrec_amd.utils.metrics import calc_ranking_results
    U, I = 20, 200
    m = M.MF(mf_config(user_num=U, item_num=I, factors=16, topk=10))
    with pytest.raises(IndexError):
        m.full_rank_users([0, U])
    indptr, items = _csr({1: [9, 3]}, U)
    with pytest.raises(ValueError, match="ascending"):
        m.full_rank_users([1], exclude=(_t(indptr), _t(items)))
    big = M.MF(mf_config(user_num=U, item_num=I, factors=16, topk=129))
    with pytest.raises(ValueError, match="cap of 128"):
        big.full_rank_users([1])
    # fewer eligible items than topk: -1 in the list, which the KPI code refuses with its own message
    few = m.full_rank_users([2], exclude={2: set(range(I - 3))}).cpu().numpy()
    assert sorted(few[0, :3].tolist()) == [I - 3, I - 2, I - 1] and np.all(few[0, 3:] == -1)
    cfg = {"logger": logging.getLogger("full-rank-test"), "res_path": str(tmp_path / "res"), "item_num": I, "topk": 10,
           "metrics": ["recall", "hit"]}
    with pytest.raises(ValueError, match="pred_ur: item id -1"):
        calc_ranking_results({2: {I - 1}}, few, [2], cfg)
    other = M.MostPop(mf_config(user_num=U, item_num=I, topk=10, algo_name="mostpop"))
    with pytest.raises(NotImplementedError, match="full_rank_users"):
        other.full_rank_users([1])
    with pytest.raises(NotImplementedError):
        M.AbstractRecommender().full_rank_users([1])
