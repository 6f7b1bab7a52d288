"""ops.full_rank_positions / model.full_rank_positions (csrc/rank_positions.hip) and utils.metrics.position_kpis /
calc_full_ranking_results (csrc/metrics_positions.hip), DESIGN.md §27, against tests/rank_positions_oracle.py: bit for
bit on exact tables, by the derived fp32 bounds and by consistency with ops.full_rank_users on real-valued ones."""
import functools
import logging

import numpy as np
import pytest
import torch

import full_rank_oracle as FO
import metrics_oracle as MO
import rank_positions_oracle as RO
from conftest import mf_config
from test_gpu_full_rank_users import _csr, _frame, _model, _model_tables, _random_rows, _same_bits, _t, _tables

pytestmark = pytest.mark.gpu
TC = 32                                                 # kFrpTc: targets of one slot
ALL = list(RO.LIST_KPIS) + ["full_auc"]


def _run(P, Q, users, targets, exclude=None, biases=None, slices=0, validate=True):
    from daisyrec_amd import ops
    ex = None if exclude is None else tuple(_t(x) for x in exclude)
    b = None if biases is None else tuple(_t(np.asarray(x, np.float32)) for x in biases)
    out = ops.full_rank_positions(_t(P), _t(Q), _t(np.asarray(users, np.int64)), tuple(_t(x) for x in targets), exclude=ex,
                                  biases=b, return_scores=True, return_eligible=True, item_slices=slices, validate=validate)
    assert all(x.is_cuda for x in out)
    assert [x.dtype for x in out] == [torch.int64, torch.int32, torch.float32, torch.int32]
    return tuple(x.cpu().numpy() for x in out)


def _sets(csr, users, I):
    """{user: set} of a CSR's rows, entries outside [0, I) dropped (they exclude nothing)"""
    return {int(u): set(int(i) for i in csr[1][csr[0][u]:csr[0][u + 1]] if 0 <= i < I) for u in set(np.asarray(users).tolist())}


def _assert_exact(P, Q, users, targets, exclude=None, biases=None, slices=0, validate=True, what=""):
    got = _run(P, Q, users, targets, exclude, biases, slices, validate)
    rows = None if exclude is None else _sets(exclude, users, Q.shape[0])
    want = RO.positions_exact(P, Q, np.asarray(users), targets, exclude=rows, biases=biases)
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), (what, np.argwhere(got[1] != want[1])[:5].ravel())
    assert _same_bits(got[2], want[2]), what
    assert np.array_equal(got[3], want[3]), (what, got[3][:8], want[3][:8])
    return got


def _target_rows(rng, U, I):
    """rows of length 0, 1, Tc - 1, Tc, Tc + 1, 3 Tc + 5 and I (every item), cut at I, in turn"""
    lens = [0, 1, TC - 1, TC, TC + 1, 3 * TC + 5, I]
    return {u: sorted(rng.choice(I, size=min(lens[u % len(lens)], I), replace=False).tolist()) for u in range(U)}


# d: k tails against the 16-deep tile, rows that are no 16-byte multiples; I and n: below, at and above one 128-item /
# 64-slot tile; slices: auto, one, several, more than there are tiles
GRID = [(1, 1, 1, 0), (3, 31, 63, 1), (16, 128, 64, 2), (64, 129, 65, 3), (130, 333, 130, 7), (64, 333, 64, 1000),
        (16, 333, 130, 0), (3, 129, 1, 2)]


@pytest.mark.parametrize("d,I,n,slices", GRID)
def test_exact_positions_scores_and_eligible(d, I, n, slices):
    rng = np.random.default_rng(d * 1000 + I + n)
    U = n + 5
    P, Q = _tables(rng, U, I, d)
    users = rng.integers(0, U, size=n)                  # any order, duplicates
    if n >= 7:
        users[:7] = np.arange(7)                        # every row length is asked for
    targets = _csr(_target_rows(rng, U, I), U)
    excl = _csr(_random_rows(rng, U, I), U)
    _assert_exact(P, Q, users, targets, what="plain")
    _assert_exact(P, Q, users, targets, exclude=excl, slices=slices, what="excluded")


def test_ties_and_zero_tables():
    rng = np.random.default_rng(3)
    U, I, d = 70, 333, 16
    P, Q = _tables(rng, U, I, d, lo=-2, hi=2)
    targets = _csr(_target_rows(rng, U, I), U)
    excl = _csr(_random_rows(rng, U, I), U)
    users = np.arange(U)
    _assert_exact(P, Q, users, targets, exclude=excl, slices=3, what="small integers")
    Z = np.zeros_like(Q)
    got = _assert_exact(P, Z, users, targets, exclude=excl, what="zeros")
    ex = _sets(excl, users, I)
    for u in (1, 5, 6):                                 # all scores equal: the eligible ids below the target
        row = targets[1][targets[0][u]:targets[0][u + 1]]
        want = [-1 if t in ex[u] else sum(1 for j in range(t) if j not in ex[u]) for t in row.tolist()]
        assert got[1][got[0][u]:got[0][u + 1]].tolist() == want


def test_biases_nan_and_inf():
    rng = np.random.default_rng(4)
    U, I, d = 20, 200, 24
    P, Q = _tables(rng, U, I, d)
    biases = (rng.integers(-50, 50, (U, 1)), rng.integers(-50, 50, (I, 1)), np.array([7.0]))
    targets = _csr({u: sorted(rng.choice(I, 6, replace=False).tolist()) for u in range(U)}, U)
    excl = _csr(_random_rows(rng, U, I), U)
    users = np.arange(U)
    _assert_exact(P, Q, users, targets, exclude=excl, biases=biases, slices=2, what="biases")
    # item 17 scores +inf for everyone (column 0 of P is positive), user 3 scores NaN everywhere
    P[:, 0] = np.minimum(np.abs(P[:, 0]), 127) + 1
    scores = FO.exact_scores(P, Q, users)
    Pn, Qn = P.copy(), Q.copy()
    Qn[17, 0] = np.inf
    Pn[3, 1] = np.nan
    scores[:, 17] = np.inf
    scores[3, :] = np.nan
    tg = {u: sorted(set(rng.choice(I, 5, replace=False).tolist()) | {17}) for u in range(U)}
    targets = _csr(tg, U)
    got = _run(Pn, Qn, users, targets, exclude=excl)
    want = RO.positions(scores, users, targets, exclude=_sets(excl, users, I))
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])
    assert np.array_equal(got[2], want[2], equal_nan=True)
    ex = _sets(excl, users, I)
    for u in range(U):
        if u != 3 and 17 not in ex[u]:
            assert got[1][got[0][u] + tg[u].index(17)] == 0          # +inf comes first
    row3 = got[1][got[0][3]:got[0][4]]                              # NaN everywhere: ascending id among the eligible
    assert row3.tolist() == [-1 if t in ex[3] else sum(1 for j in range(t) if j not in ex[3]) for t in tg[3]]


def test_exclusion_edges_and_bad_targets():
    rng = np.random.default_rng(5)
    U, I, d = 12, 150, 16
    P, Q = _tables(rng, U, I, d)
    excl_rows = {0: [], 1: list(range(I)), 2: [3, 4, 140], 3: sorted(rng.choice(I, 40, replace=False).tolist())}
    tg = {0: [0, 149], 1: [5, 77], 2: [3, 4, 5, 140, 141], 3: list(range(0, I, 7)), 4: [9]}
    users = np.array([0, 1, 2, 3, 4, 2])
    got = _assert_exact(P, Q, users, _csr(tg, U), exclude=_csr(excl_rows, U), what="edges")
    assert got[1][2:4].tolist() == [-1, -1] and got[3].tolist()[:3] == [I, 0, I - 3]        # everything excluded
    assert (got[1][4:9] < 0).tolist() == [True, True, False, True, False]                   # targets inside the row
    assert np.all(np.isneginf(got[2][got[1] < 0]))
    # a target >= I with validate=False: compared and range-checked only, never an index
    bad = {0: [0, 149, I, I + 1000], 2: [5, 2 ** 31 - 1]}
    indptr, items = _csr(bad, U)
    got = _assert_exact(P, Q, np.array([0, 2]), (indptr, items), exclude=_csr(excl_rows, U), validate=False, what="bad ids")
    assert got[1][2:4].tolist() == [-1, -1] and got[1][5] == -1 and got[1][4] >= 0


def test_duplicate_users_and_the_ops_surface():
    from daisyrec_amd import ops
    rng = np.random.default_rng(6)
    U, I, d = 30, 300, 16
    P, Q = _tables(rng, U, I, d)
    tg = _csr({u: sorted(rng.choice(I, 1 + u % 5, replace=False).tolist()) for u in range(U)}, U)
    ex = _csr(_random_rows(rng, U, I), U)
    users = np.array([4, 9, 4, 4, 0, 9])
    got = _assert_exact(P, Q, users, tg, exclude=ex, what="duplicates")
    rows = [got[1][got[0][b]:got[0][b + 1]].tolist() for b in range(len(users))]
    assert rows[0] == rows[2] == rows[3] and rows[1] == rows[5]
    Pd, Qd, tgd = _t(P), _t(Q), tuple(_t(x) for x in tg)
    out = ops.full_rank_positions(Pd, Qd, torch.tensor([4, 9]), tgd, exclude=tuple(_t(x) for x in ex))
    assert len(out) == 2 and out[1].tolist() == rows[0] + rows[1]
    empty = ops.full_rank_positions(Pd, Qd, torch.zeros(0, dtype=torch.int64), tgd, return_scores=True, return_eligible=True)
    assert [tuple(x.shape) for x in empty] == [(1,), (0,), (0,), (0,)]
    none = _csr({}, U)                                           # T = 0: nothing is ranked, the eligible counts remain
    oi, pos, el = ops.full_rank_positions(Pd, Qd, torch.tensor([4, 9]), tuple(_t(x) for x in none), return_eligible=True)
    assert oi.tolist() == [0, 0, 0] and pos.numel() == 0 and el.tolist() == [I, I]
    with pytest.raises(IndexError):
        ops.full_rank_positions(Pd, Qd, torch.tensor([0, U]), tgd)
    for rows_bad, text in (({1: [9, 3]}, "ascending"), ({1: [3, 3]}, "twice")):
        with pytest.raises(ValueError, match=text):
            ops.full_rank_positions(Pd, Qd, torch.tensor([1]), tuple(_t(x) for x in _csr(rows_bad, U)))
    with pytest.raises(ValueError, match="indptr"):
        ops.full_rank_positions(Pd, Qd, torch.tensor([1]), (tgd[0][:-1], tgd[1]))
    with pytest.raises(ValueError, match="exclude"):
        ops.full_rank_positions(Pd, Qd, torch.tensor([1]), tgd, exclude=tuple(_t(x) for x in _csr({1: [9, 3]}, U)))


# ---- real-valued tables --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _real():
    """300 x 1500 x 64, about 8 targets per user outside the exclusion; five users keep fewer than 1000 eligible items"""
    rng = np.random.default_rng(2027)
    U, I, d = 300, 1500, 64
    P = rng.normal(0, 0.1, (U, d)).astype(np.float32)
    Q = rng.normal(0, 0.1, (I, d)).astype(np.float32)
    ex = _random_rows(rng, U, I, share=0.1)
    for u in range(5):
        ex[u] = sorted(rng.choice(I, 1000, replace=False).tolist())
    tg = {}
    for u in range(U):
        free = np.setdiff1d(np.arange(I), ex[u])
        tg[u] = sorted(rng.choice(free, int(rng.integers(4, 13)), replace=False).tolist())
    users = rng.permutation(U)
    return P, Q, users, _csr(tg, U), _csr(ex, U), tg


@functools.lru_cache(maxsize=None)
def _real_run():
    P, Q, users, tg, ex, _ = _real()
    return _run(P, Q, users, tg, exclude=ex)


def test_real_tables_agree_with_full_rank_users():
    """ids[b, pos] == t for every target with pos < topk, no other target is listed, and the score bits agree"""
    from daisyrec_amd import ops
    P, Q, users, tg, ex, rows = _real()
    oi, pos, sc, el = _real_run()
    assert np.all(pos >= 0)                                      # no target is skipped
    ids, lsc = ops.full_rank_users(_t(P), _t(Q), _t(users), 128, exclude=tuple(_t(x) for x in ex), return_scores=True)
    ids, lsc = ids.cpu().numpy(), lsc.cpu().numpy()
    listed = 0
    for b, u in enumerate(users.tolist()):
        p, row = pos[oi[b]:oi[b + 1]], np.array(rows[u])
        inside = p < 128
        assert np.array_equal(ids[b, p[inside]], row[inside]), b
        assert _same_bits(lsc[b, p[inside]], sc[oi[b]:oi[b + 1]][inside]), b
        assert not np.isin(row[~inside], ids[b]).any(), b
        listed += int(inside.sum())
    assert listed > 50                                           # (random tables: about 128 / 1350 of 2400 targets)
    assert np.array_equal(el, np.array([Q.shape[0] - len(set(ex[1][ex[0][u]:ex[0][u + 1]].tolist())) for u in users]))


def test_real_tables_within_the_fp32_bounds():
    P, Q, users, tg, ex, _ = _real()
    _, pos, _, _ = _real_run()
    lo, hi = RO.position_bounds(P, Q, users, tg, exclude=ex)
    assert np.all((lo <= pos) & (pos <= hi)), np.argwhere((lo > pos) | (pos > hi))[:5].ravel()


def test_real_tables_same_bits_across_runs_and_slices():
    P, Q, users, tg, ex, _ = _real()
    first = _real_run()
    for slices in (0, 1, 2, 3, 7, 1000):
        again = _run(P, Q, users, tg, exclude=ex, slices=slices)
        assert all(np.array_equal(a, b) for a, b in zip(first[:2] + first[3:], again[:2] + again[3:])), slices
        assert _same_bits(first[2], again[2]), slices


# ---- KPIs ----------------------------------------------------------------------------------------------------------------
def test_kpis_equal_the_list_kpis_up_to_the_cap():
    """cutoffs <= 128: position_kpis against ranking_kpis on full_rank_users' lists - precision, recall, hit, mrr and auc
    bit for bit, map, ndcg and f1 within metrics_oracle's bound (another summation order)"""
    from daisyrec_amd import ops
    from daisyrec_amd.utils import metrics as M
    P, Q, users, tg, ex, rows = _real()
    oi, pos, _, el = _real_run()
    cutoffs = [1, 5, 10, 50, 128]
    ids = ops.full_rank_users(_t(P), _t(Q), _t(users), 128, exclude=tuple(_t(x) for x in ex))
    test_ur = {u: set(r) for u, r in rows.items()}
    ref = M.ranking_kpis(ids, test_ur, users, cutoffs, list(RO.LIST_KPIS), item_num=Q.shape[0], per_user=True)
    got = M.position_kpis(_t(oi), _t(pos), None, _t(el), cutoffs, list(RO.LIST_KPIS), per_user=True)
    assert got["cutoffs"] == cutoffs and got["coverage_counts"] is None
    for m in MO.BITWISE:
        assert np.array_equal(got["per_user"][m], ref["per_user"][m], equal_nan=True), m
        assert np.array_equal(got["means"][m], ref["means"][m], equal_nan=True), m
    MO.check_regimes(got["per_user"], got["means"], ref["per_user"], ref["means"], cutoffs, False, what="positions vs lists: ")
    again = M.position_kpis(_t(oi), _t(pos), None, _t(el), cutoffs, list(RO.LIST_KPIS), per_user=True)
    for m in RO.LIST_KPIS:
        assert np.array_equal(got["per_user"][m], again["per_user"][m], equal_nan=True)
        assert np.array_equal(got["means"][m], again["means"][m], equal_nan=True)
    only = M.position_kpis(_t(oi), _t(pos), None, _t(el), [10], ["ndcg", "recall"])
    assert list(only["means"]) == ["recall", "ndcg"] and only["per_user"] is None
    assert np.array_equal(only["means"]["ndcg"], got["means"]["ndcg"][2:3])
    for name in ("popularity", "diversity", "coverage"):
        with pytest.raises(ValueError, match="full_rank_users"):
            M.position_kpis(_t(oi), _t(pos), None, _t(el), [10], ["recall", name])
    with pytest.raises(ValueError, match="Invalid metric name"):
        M.position_kpis(_t(oi), _t(pos), None, _t(el), [10], ["recal"])
    with pytest.raises(ValueError, match="strictly ascending"):
        M.position_kpis(_t(oi), _t(pos), None, _t(el), [10, 10], ["recall"])


def test_kpis_beyond_the_cap_and_full_auc_against_the_oracle():
    """exact tables: cutoffs 200 and 1000 - above the list cap, 1000 above the eligible items of some users - and
    full_auc, against metrics_oracle on the oracle's own full sort; long rows, unranked targets and a row of one"""
    from daisyrec_amd.utils import metrics as M
    rng = np.random.default_rng(8)
    U, I, d = 40, 1200, 16
    P, Q = _tables(rng, U, I, d)
    ex = _random_rows(rng, U, I, share=0.1)
    for u in range(4):
        ex[u] = sorted(rng.choice(I, 600 + 150 * u, replace=False).tolist())      # 600 .. 150 eligible items
    tg = {u: sorted(rng.choice(I, 1 + (7 * u) % 90, replace=False).tolist()) for u in range(U)}   # some inside the exclusion
    users = np.concatenate([np.arange(U), [3, 3]])
    cutoffs = [1, 10, 128, 200, 1000]
    oi, pos, _, el = _assert_exact(P, Q, users, _csr(tg, U), exclude=_csr(ex, U), what="kpi tables")
    assert (pos < 0).any() and el.min() < 200
    _, _, _, _, lists = RO.positions_exact(P, Q, users, tg, exclude=ex)
    rows = [np.array(tg[u], np.int64) for u in users.tolist()]
    ref_per, ref_means = RO.kpis_from_lists(lists, rows, cutoffs, ALL)
    got = M.position_kpis(_t(oi), _t(pos), None, _t(el), cutoffs, ALL, per_user=True)
    for m in MO.BITWISE + ("full_auc",):
        assert np.array_equal(got["per_user"][m], ref_per[m], equal_nan=True), m
    lists_only = {m: ref_per[m] for m in RO.LIST_KPIS}
    MO.check_regimes(got["per_user"], got["means"], lists_only, {m: ref_means[m] for m in RO.LIST_KPIS}, cutoffs, False,
                     what="positions vs oracle: ")
    assert np.array_equal(got["per_user"]["full_auc"][0], got["per_user"]["full_auc"][-1], equal_nan=True)      # the same at every cutoff
    assert np.isclose(got["means"]["full_auc"][0], ref_means["full_auc"][0], rtol=0, atol=4 * len(users) * MO.U64,
                      equal_nan=True)
    # gt_len given: recall's denominator
    twice = M.position_kpis(_t(oi), _t(pos), 2 * np.diff(oi), _t(el), [200], ["recall"], per_user=True)
    assert np.array_equal(twice["per_user"]["recall"][0] * 2, got["per_user"]["recall"][3])


# ---- model level ---------------------------------------------------------------------------------------------------------
def _cfg(tmp_path, I, topk, metrics):
    return {"logger": logging.getLogger("full-rank-positions-test"), "res_path": str(tmp_path / "res"), "item_num": I,
            "topk": topk, "metrics": metrics}


@pytest.mark.parametrize("name", ["mf", "fm", "lightgcn", "ngcf", "item2vec"])
def test_calc_full_ranking_results(name, tmp_path):
    from daisyrec_amd.utils.metrics import calc_full_ranking_results, calc_ranking_results
    from daisyrec_amd.utils.utils import user_csr
    rng = np.random.default_rng(27)
    U, I, topk = 300, 400, 60
    tr, train_ur, test_ur = _frame(U, I, rng, n_train=6000, n_test=900)
    short = 7                                                    # user 7 keeps 20 eligible items: fewer than topk
    keep = set(rng.choice(I, 20, replace=False).tolist())
    train_ur[short] = set(range(I)) - keep
    test_ur[short] = set(sorted(keep)[:3])
    tr = np.array(sorted((u, i) for u, s in train_ur.items() for i in s), np.int64)
    m = _model(name, U, I, tr, train_ur, topk)
    m.eval()
    metrics = ["recall", "mrr", "ndcg", "hit", "precision", "map", "full_auc"]
    got = calc_full_ranking_results(m, test_ur, train_ur, _cfg(tmp_path, I, topk, metrics))
    assert list(got.columns) == ["KPI@K", 1, 5, 10, 20, 30, 50, 60] and len(got) == len(metrics)
    assert got["KPI@K"].tolist()[:5] == ["Recall", "MRR", "NDCG", "Hit Ratio", "Precision"]
    # the frame is the oracle's on the positions of the same call, whose own checks are the tests above
    users = np.asarray(list(test_ur), np.int64)
    oi, pos, sc, el = m.full_rank_positions(users, user_csr(np.array([(u, i) for u, s in test_ur.items() for i in s]).T, U),
                                            exclude=user_csr(tr.T, U), return_scores=True, return_eligible=True)
    oi, pos, el = oi.cpu().numpy(), pos.cpu().numpy(), el.cpu().numpy()
    assert el[list(test_ur).index(short)] == 20 and np.all(pos >= 0)
    Pm, Qm, biases = _model_tables(name, m)
    lo, hi = RO.position_bounds(Pm, Qm, users, test_ur, exclude=train_ur, biases=biases)
    assert np.all((lo <= pos) & (pos <= hi))
    ks = [1, 5, 10, 20, 30, 50, 60]
    ref_per, ref_means = RO.kpis_from_positions(oi, pos, None, el, ks, metrics)
    for r, mname in enumerate(metrics):
        row = got.iloc[r, 1:].to_numpy(dtype=np.float64)
        tol = 0.0 if mname == "hit" else 8 * (len(users) + 60) * MO.U64 * np.abs(ref_means[mname]).max()
        assert np.all(np.abs(row - ref_means[mname]) <= tol), (mname, row, ref_means[mname])
    # without the short user the list path is open, and the two frames agree
    del test_ur[short]
    test_u = list(test_ur)
    lists = m.full_rank_users(test_u, exclude=train_ur)
    bitwise = ["recall", "mrr", "hit", "precision"]
    a = calc_full_ranking_results(m, test_ur, train_ur, _cfg(tmp_path, I, topk, bitwise))
    b = calc_ranking_results(test_ur, lists, test_u, _cfg(tmp_path, I, topk, bitwise))
    assert a.equals(b)


def test_model_errors(tmp_path):
    from daisyrec_amd import model as M
    from daisyrec_amd.utils.metrics import calc_full_ranking_results
    U, I = 20, 200
    m = M.MF(mf_config(user_num=U, item_num=I, factors=16, topk=10))
    with pytest.raises(IndexError):
        m.full_rank_positions([0, U], {0: {1}})
    with pytest.raises(ValueError, match="no ground truth"):
        calc_full_ranking_results(m, {1: {3}, 2: set()}, {1: {4}}, _cfg(tmp_path, I, 10, ["recall"]))
    with pytest.raises(ValueError, match="Invalid metric name"):
        calc_full_ranking_results(m, {1: {3}}, {1: {4}}, _cfg(tmp_path, I, 10, ["recal"]))
    with pytest.raises(ValueError, match="full_rank_users"):
        calc_full_ranking_results(m, {1: {3}}, {1: {4}}, _cfg(tmp_path, I, 10, ["coverage"]))
    # config['topk'] above the list cap, a user with 3 eligible items
    res = calc_full_ranking_results(m, {1: {3}, 2: {I - 1}}, {2: set(range(I - 3))}, _cfg(tmp_path, I, 500, ["recall", "hit"]))
    assert list(res.columns) == ["KPI@K", 1, 5, 10, 20, 30, 50, 500] and res[500].tolist() == [1.0, 1.0]
    assert res[5].tolist()[1] >= 0.5                             # user 2's truth is among its 3 eligible items
    ease = M.EASE(mf_config(algo_name="ease", reg=50.0, user_num=U, item_num=I, topk=10))
    neumf = M.NeuMF(mf_config(user_num=U, item_num=I, factors=8, num_layers=2, dropout=0.0, model_name="NeuMF", GMF_model=None,
                              MLP_model=None, algo_name="neumf", topk=10))
    for other in (ease, neumf, M.AbstractRecommender()):
        with pytest.raises(NotImplementedError, match="full_rank_positions"):
            other.full_rank_positions([1], {1: {3}})
