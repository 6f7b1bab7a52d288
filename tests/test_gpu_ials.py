"""iALS on the device (csrc/ials.hip): the Gram matrix, the normal equations and the objective against
exact integer / dyadic arithmetic, the solves against constructions whose every Cholesky step is exact, the half-sweep
against the numpy oracle (tests/ials_oracle.py) under a tolerance derived from the systems' condition, the bad-pivot status
path, and the model end to end through IALS.fit(DataFrame) and fold_in.  No tolerance comes from the device's own result."""
import functools
import logging

import numpy as np
import pytest
import torch

import ials_oracle as O
from conftest import mf_config
from test_oracle_ials import EXACT_DIMS, exact_case, model_case, model_csr

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIMS = [1, 8, 24, 64, 100, 128]                     # one tile, part of one, an odd tile count, the flagship, a ragged tile, the limit
CONFIGS = [(10.0, 0.1), (40.0, 0.01), (1.0, 0.05)]  # (alpha, reg)
I_ITEMS = 300                                       # above the longest listed row (257)


def _dev(a, dtype=None):
    t = torch.as_tensor(np.array(a))
    return t.to(DEV, dtype) if dtype is not None else t.to(DEV)


def _csr(csr):
    return _dev(csr[0], torch.int64), _dev(csr[1], torch.int32), _dev(csr[2], torch.float32)


def _np(t):
    return t.cpu().numpy()


# ---- 1. exact systems ------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def int_case(d, long_row=False):
    """integer tables with entries in [-3, 3], integer ratings 1..5 and, in exact int64 arithmetic at alpha = 1/2, reg = 2:
    G, 2 A_u, 2 b_u and twice the objective"""
    rng = np.random.default_rng(1000 + d + long_row)
    I = 4000 if long_row else I_ITEMS
    lengths = [3000, 2] if long_row else list(O.ROW_LENGTHS)
    csr = O.csr_of_lengths(lengths, I, rng)
    row_ptr, col, val = csr
    Y = rng.integers(-3, 4, (I, d))
    X = rng.integers(-3, 4, (len(lengths), d))
    G = Y.T @ Y
    A2, b2, obj2 = [], [], 0
    for u in range(len(lengths)):
        Yu = Y[col[row_ptr[u]:row_ptr[u + 1]]]
        r = val[row_ptr[u]:row_ptr[u + 1]].astype(np.int64)
        A2.append(2 * G + 4 * np.eye(d, dtype=np.int64) + (Yu * r[:, None]).T @ Yu)
        b2.append(((2 + r)[:, None] * Yu).sum(0))
        s = Yu @ X[u]
        obj2 += int(2 * (X[u] @ G @ X[u]) + ((2 + r) * (1 - s) ** 2 - 2 * s ** 2).sum())
    obj2 += 4 * int((X ** 2).sum() + (Y ** 2).sum())
    for a in (Y, X, G):
        a.setflags(write=False)
    return csr, Y, X, G, np.array(A2), np.array(b2), obj2


@pytest.mark.parametrize("d,long_row", [(d, False) for d in DIMS] + [(8, True)])
def test_the_systems_and_the_gram_matrix_are_exact_on_integer_operands(d, long_row):
    """every term is a small dyadic number, so the order of the sums does not matter: equality, not a tolerance"""
    from daisyrec_amd import ops
    csr, Y, X, G, A2, b2, _ = int_case(d, long_row)
    Yd = _dev(Y, torch.float32)
    Gd = ops.ials_gram(Yd)
    assert np.array_equal(_np(Gd), G.astype(np.float64))
    _, info, A, b = ops.ials_half_sweep(_csr(csr), Yd, 0.5, 2.0, dump=True)
    assert int(info.item()) == 0
    assert np.array_equal(2 * _np(A), A2.astype(np.float64))
    assert np.array_equal(2 * _np(b), b2.astype(np.float64))


# ---- 2. exact solves -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", sorted(EXACT_DIMS))
def test_the_solve_is_exact_where_every_cholesky_step_is(d):
    """Y = L^T, reg = alpha = 0, rows = subsets with rating 1: A = L L^T in integers, the factor is L, z = 1_S and
    x = L^-T 1_S is dyadic and fits fp32 (asserted on the CPU first): the kernel's output equals it"""
    from daisyrec_amd import ops
    L, csr, want, ok = exact_case(d)
    assert ok and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    X, info = ops.ials_half_sweep(_csr(csr), _dev(L.T.copy(), torch.float32), 0.0, 0.0)
    assert int(info.item()) == 0
    assert np.array_equal(_np(X), want.astype(np.float32))


# ---- 3. the half-sweep against the oracle ------------------------------------------------------------------------------------
def _bound(want32):
    """|got - want| <= ulp32(want) + 1e-9 max|want_row|: under cond(A) <= 1e4 two fp64 solutions differ by about
    cond d 2^-52 ~ 3e-10 of the row's largest element, so their fp32 roundings differ by one ulp at the most"""
    w = np.abs(want32.astype(np.float64))
    return np.spacing(np.abs(want32)).astype(np.float64) + 1e-9 * w.max(axis=1, keepdims=True)


@functools.lru_cache(None)
def float_case(d, alpha, reg, rows):
    """random fp32 tables (normal, scale 0.1), ratings 1..5; rows = 0: the listed row lengths, else that many rows of
    random length below 40"""
    rng = np.random.default_rng(2000 + 7 * d + rows)
    lengths = list(O.ROW_LENGTHS) if rows == 0 else rng.integers(0, 40, rows).tolist()
    if rows == 1:
        lengths = [17]
    csr = O.csr_of_lengths(lengths, I_ITEMS, rng)
    Y = (0.1 * rng.standard_normal((I_ITEMS, d))).astype(np.float32)
    A, _ = O.normal_equations(*csr, Y, alpha, reg)
    cond = max(np.linalg.cond(a) for a in A)
    want = O.half_sweep(*csr, Y, alpha, reg)
    Y.setflags(write=False)
    want.setflags(write=False)
    return csr, Y, want, cond


SWEEP_CASES = [(d, a, r, 0) for d in DIMS for a, r in CONFIGS] + [(d, 10.0, 0.1, n) for d in (24, 64, 128) for n in (1, 7, 300)]


@pytest.mark.parametrize("d,alpha,reg,rows", SWEEP_CASES)
def test_half_sweep_against_the_oracle(d, alpha, reg, rows):
    from daisyrec_amd import ops
    csr, Y, want, cond = float_case(d, alpha, reg, rows)
    assert cond <= 1e4, cond                                     # a condition on the inputs, not on the result
    X, info = ops.ials_half_sweep(_csr(csr), _dev(Y), alpha, reg)
    got = _np(X)
    assert int(info.item()) == 0
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"d={d} alpha={alpha} reg={reg} rows={len(want)}: cond {cond:.3g}, differing fp32 elements "
          f"{int((got != want).sum())} of {want.size}, max err / bound {np.max(err / _bound(want)):.3g}")
    assert np.all(err <= _bound(want))
    empty = np.diff(csr[0]) == 0
    assert not got[empty].any()


@pytest.mark.parametrize("d", [24, 64, 100])
def test_half_sweep_is_reproducible_and_independent_of_g_and_the_row_pitch(d):
    from daisyrec_amd import ops
    csr, Y, want, _ = float_case(d, 10.0, 0.1, 0)
    cd, Yd = _csr(csr), _dev(Y)
    X0, _ = ops.ials_half_sweep(cd, Yd, 10.0, 0.1)
    X1, _ = ops.ials_half_sweep(cd, Yd, 10.0, 0.1)
    assert torch.equal(X0, X1)
    G = ops.ials_gram(Yd)
    assert torch.equal(G, G.T) and torch.equal(G, ops.ials_gram(Yd))
    assert torch.equal(ops.ials_half_sweep(cd, Yd, 10.0, 0.1, G=G)[0], X0)
    pitch = (d + 31) // 32 * 32 + 32
    wide = torch.full((I_ITEMS, pitch), 7.0, device=DEV)        # what lies between the rows must not matter
    wide[:, :d] = Yd
    assert torch.equal(ops.ials_gram(wide[:, :d]), G)
    out = torch.full((len(want), pitch), -1.0, device=DEV)
    X2, _ = ops.ials_half_sweep(cd, wide[:, :d], 10.0, 0.1, out=out[:, :d])
    assert torch.equal(X2, X0) and bool((out[:, d:] == -1.0).all())


def test_half_sweep_argument_errors():
    from daisyrec_amd import ops
    csr, Y, _, _ = float_case(8, 10.0, 0.1, 0)
    row_ptr, col, val = csr
    bad = col.copy()
    bad[5] = I_ITEMS
    with pytest.raises(IndexError):
        ops.ials_half_sweep(_csr((row_ptr, bad, val)), _dev(Y), 10.0, 0.1)
    bad[5] = -1
    with pytest.raises(IndexError):
        ops.ials_half_sweep(_csr((row_ptr, bad, val)), _dev(Y), 10.0, 0.1)
    # validate=False trusts the ids; the kernel leaves such an entry out and reads nothing outside the table
    X, info = ops.ials_half_sweep(_csr((row_ptr, bad, val)), _dev(Y), 10.0, 0.1, validate=False)
    keep = np.ones(len(col), bool)
    keep[5] = False
    ptr2 = row_ptr.copy()
    ptr2[np.searchsorted(row_ptr, 5, side="right"):] -= 1
    want = O.half_sweep(ptr2, col[keep], val[keep], Y, 10.0, 0.1)
    assert np.all(np.abs(_np(X).astype(np.float64) - want) <= _bound(want))
    with pytest.raises(ValueError, match="128"):
        ops.ials_half_sweep(_csr(csr), torch.zeros(I_ITEMS, 129, device=DEV), 10.0, 0.1)
    with pytest.raises(ValueError, match="128"):
        ops.ials_gram(torch.zeros(I_ITEMS, 129, device=DEV))
    with pytest.raises(ValueError):
        ops.ials_half_sweep(_csr(csr), _dev(Y), float("nan"), 0.1)
    with pytest.raises(ValueError):
        ops.ials_half_sweep(_csr(csr), _dev(Y), 10.0, 0.1, G=torch.zeros(4, 4, dtype=torch.float64, device=DEV))


# ---- 4. a bad pivot ----------------------------------------------------------------------------------------------------------
def test_a_bad_pivot_is_reported_not_solved():
    """an item table with a zero column at reg = 0: the 2 x 2 system of every row with an entry has a zero pivot - rows 1 and
    3 of five here; info names the smaller one, both are NaN, the (empty) others are the oracle's zeros"""
    from daisyrec_amd import ops
    Y = np.array([[1, 0], [2, 0], [3, 0]], np.float32)
    row_ptr = np.array([0, 0, 2, 2, 3, 3], np.int64)
    csr = (row_ptr, np.array([0, 2, 1], np.int32), np.array([1, 2, 3], np.float32))
    X, info = ops.ials_half_sweep(_csr(csr), _dev(Y), 1.0, 0.0)
    got = _np(X)
    assert int(info.item()) == 2
    assert np.isnan(got[[1, 3]]).all() and not got[[0, 2, 4]].any()
    # with reg > 0 the same rows are solved
    X, info = ops.ials_half_sweep(_csr(csr), _dev(Y), 1.0, 0.5)
    want = O.half_sweep(*csr, Y, 1.0, 0.5)
    assert int(info.item()) == 0 and np.all(np.abs(_np(X).astype(np.float64) - want) <= _bound(want))


def test_an_indefinite_system_is_reported_and_the_other_rows_are_solved():
    """weights below zero (ratings the model refuses, the operator does not) make A indefinite in rows 4 and 2 of five;
    the other three rows are the oracle's"""
    from daisyrec_amd import ops
    rng = np.random.default_rng(4)
    Y = rng.integers(-2, 3, (12, 2)).astype(np.float32)
    csr = list(O.csr_of_lengths([3, 4, 2, 5, 3], 12, rng))
    for u in (2, 4):
        csr[2][csr[0][u]:csr[0][u + 1]] = -50.0
    A, _ = O.normal_equations(*csr, Y, 1.0, 0.0)
    assert [bool(np.linalg.eigvalsh(a).min() < 0) for a in A] == [False, False, True, False, True]
    X, info, Ad, _ = ops.ials_half_sweep(_csr(csr), _dev(Y), 1.0, 0.0, dump=True)
    assert np.array_equal(_np(Ad), A)                            # small integers: the dump shows the offending systems
    got = _np(X)
    assert int(info.item()) == 3
    assert np.isnan(got[[2, 4]]).all()
    want = O.half_sweep(*csr, Y, 1.0, 0.0)
    assert np.all(np.abs(got[[0, 1, 3]].astype(np.float64) - want[[0, 1, 3]]) <= _bound(want[[0, 1, 3]]))


# ---- 5. the objective --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,long_row", [(d, False) for d in DIMS] + [(8, True)])
def test_objective_is_exact_on_integer_operands(d, long_row):
    from daisyrec_amd import ops
    csr, Y, X, _, _, _, obj2 = int_case(d, long_row)
    assert obj2 < 1 << 52
    got = ops.ials_objective(_csr(csr), _dev(X, torch.float32), _dev(Y, torch.float32), 0.5, 2.0)
    assert got.dtype == torch.float64 and got.dim() == 0
    assert 2 * float(got.item()) == float(obj2)


@pytest.mark.parametrize("d,alpha,reg,rows", [(d, a, r, 0) for d in DIMS for a, r in CONFIGS] + [(64, 10.0, 0.1, 300)])
def test_objective_against_the_oracle(d, alpha, reg, rows):
    """1e-12 relative: fp64 summation round-off.  The largest case adds 300 rows' x^T G x (64^2 products each), 5 900
    entry terms of 64 products and the two norms: under 2e6 products of one sign pattern per partial sum chain of at most
    1e5 terms, each rounding 1.1e-16 relative - the chains' random-walk error is far below 1e5 * 1.1e-16 = 1.1e-11 and the
    terms are positive or cancel by a bounded factor (c (1 - s)^2 against s^2, |s| < 1)"""
    from daisyrec_amd import ops
    csr, Y, want_x, _ = float_case(d, alpha, reg, rows)
    X = np.array(want_x)
    want = O.objective(*csr, X, Y, alpha, reg)
    got = ops.ials_objective(_csr(csr), _dev(X), _dev(Y), alpha, reg)
    again = ops.ials_objective(_csr(csr), _dev(X), _dev(Y), alpha, reg)
    print(f"d={d} alpha={alpha} reg={reg}: objective {want!r}, relative difference {abs(got.item() - want) / abs(want):.3g}")
    assert abs(got.item() - want) <= 1e-12 * abs(want)
    assert torch.equal(got, again)


# ---- 6. the model ------------------------------------------------------------------------------------------------------------
ALPHA, REG, EPOCHS = 10.0, 0.1, 3


def ials_config(**over):
    cfg = mf_config(algo_name="ials", user_num=40, item_num=60, factors=8, reg=REG, alpha=ALPHA, epochs=EPOCHS, topk=10)
    cfg.update(over)
    return cfg


def _frame():
    import pandas as pd
    _, _, users, items, ratings = model_case()
    return pd.DataFrame({"user": users, "item": items, "rating": ratings})


@functools.lru_cache(None)
def fitted():
    """(model, its initial tables as numpy arrays): one fit shared by the tests below, which do not change it"""
    from daisyrec_amd.model import IALS
    torch.manual_seed(7)
    model = IALS(ials_config())
    P0, Q0 = model.embed_user.weight.detach().numpy().copy(), model.embed_item.weight.detach().numpy().copy()
    model.fit(_frame())
    return model, P0, Q0


def test_fit_is_the_chain_of_half_sweeps_and_the_objective_falls():
    from daisyrec_amd import ops
    model, P0, Q0 = fitted()
    _, _, users, items, ratings = model_case()
    u, i, r = _dev(users), _dev(items), _dev(ratings)
    csr, csr_t = ops.slim_csr(u, i, r, 40, 60), ops.slim_csr(i, u, r, 60, 40)
    want_csr = model_csr()
    assert all(np.array_equal(_np(a), b) for a, b in zip(csr, want_csr))
    P, Q, losses = _dev(P0), _dev(Q0), []
    for _ in range(EPOCHS):
        P, _ = ops.ials_half_sweep(csr, Q, ALPHA, REG)
        Q, _ = ops.ials_half_sweep(csr_t, P, ALPHA, REG)
        losses.append(float(ops.ials_objective(csr, P, Q, ALPHA, REG).item()))
    assert torch.equal(model.embed_user.weight.data, P) and torch.equal(model.embed_item.weight.data, Q)
    assert model.loss_history == losses
    assert losses[0] > losses[1] > losses[2]
    assert model.fit_info["epochs_run"] == EPOCHS and model.fit_info["nnz"] == len(want_csr[1])


def test_fit_against_the_oracle_within_its_own_sensitivity():
    """the yardstick is the oracle's own sensitivity to the rounding of the tables between half-sweeps: the largest
    element-wise deviation between the oracle that rounds them to fp32 and the one that keeps fp64 throughout.  The
    kernels' tables and the rounding oracle's are each one rounding path away from the same exact iterate: 2 x."""
    model, P0, Q0 = fitted()
    csr = model_csr()
    P32, Q32, l32 = O.fit(*csr, P0, Q0, ALPHA, REG, EPOCHS, round32=True)
    P64, Q64, _ = O.fit(*csr, P0, Q0, ALPHA, REG, EPOCHS, round32=False)
    yard = max(np.abs(P32 - P64).max(), np.abs(Q32 - Q64).max())
    dev = max(np.abs(_np(model.embed_user.weight.data) - P32).max(), np.abs(_np(model.embed_item.weight.data) - Q32).max())
    print(f"oracle sensitivity {yard:.3g}, kernels against the rounding oracle {dev:.3g}")
    assert yard > 0 and dev <= 2 * yard
    assert np.allclose(model.loss_history, l32, rtol=1e-6, atol=0)


def test_scoring_is_what_mf_calls_on_the_tables(tmp_path):
    from daisyrec_amd import ops
    from daisyrec_amd.utils.metrics import calc_full_ranking_results
    from daisyrec_amd.utils.utils import _ur_pairs, user_csr
    model, _, _ = fitted()
    P, Q = model.embed_user.weight.data, model.embed_item.weight.data
    rng = np.random.default_rng(9)
    assert model.predict(3, 5) == float(ops.mf_predict(P, Q, _dev([3]), _dev([5])).item())
    us, cands = torch.arange(6), torch.from_numpy(rng.integers(0, 60, (6, 20)))
    got = model.rank([(us, cands)])
    assert got.dtype == np.float32
    assert np.array_equal(got, _np(ops.mf_rank_topk(P, Q, us.to(DEV), cands.to(DEV), 10)).astype(np.float32))
    assert np.array_equal(model.full_rank(4), _np(ops.mf_full_rank(P, Q, 4, 10)))
    _, _, users, items, _ = model_case()
    train_ur = {u: set(items[users == u].tolist()) for u in range(40)}
    train = user_csr(_ur_pairs(train_ur), 40, DEV)
    every = torch.arange(40, device=DEV)
    ids, sc = model.full_rank_users(every, exclude=train, return_scores=True)
    ids2, sc2 = ops.full_rank_users(P, Q, every, 10, exclude=train, return_scores=True)
    assert torch.equal(ids, ids2) and torch.equal(sc, sc2)
    test_ur = {u: {int(rng.integers(57, 60))} for u in range(40)}            # items 57..59 are in no training row
    tg = user_csr(_ur_pairs(test_ur), 40, DEV)
    a = model.full_rank_positions(every, test_ur, exclude=train_ur, return_eligible=True)
    b = ops.full_rank_positions(P, Q, every, tg, exclude=train, return_eligible=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    cfg = {"logger": logging.getLogger("ials-test"), "res_path": str(tmp_path / "res"), "item_num": 60, "topk": 10,
           "metrics": ["recall", "ndcg", "full_auc"]}
    res = calc_full_ranking_results(model, test_ur, train_ur, cfg)
    assert list(res.columns) == ["KPI@K", 1, 5, 10] and len(res) == 3 and np.isfinite(res[10].to_numpy()).all()


def test_state_dict_round_trip():
    from daisyrec_amd.model import IALS
    model, _, _ = fitted()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    other = IALS(ials_config())
    with pytest.raises(RuntimeError, match="fit"):
        other.full_rank(0)
    other.load_state_dict(state)
    assert torch.equal(other.embed_user.weight.data.cpu(), model.embed_user.weight.data.cpu())
    assert np.array_equal(other.full_rank(4), model.full_rank(4))


def test_early_stop_ends_a_fit_whose_objective_has_stalled():
    """under a heavy regulariser the sweeps contract fast: the oracle says after how many epochs two successive objectives
    are within 1e-5, and the model stops there"""
    from daisyrec_amd.model import IALS
    torch.manual_seed(8)
    model = IALS(ials_config(reg=50.0, alpha=1.0, epochs=60, early_stop=True))
    P0, Q0 = model.embed_user.weight.detach().numpy().copy(), model.embed_item.weight.detach().numpy().copy()
    losses = O.fit(*model_csr(), P0, Q0, 1.0, 50.0, 60)[2]
    stalled = [k for k in range(1, 60) if abs(losses[k] - losses[k - 1]) < 1e-5]
    assert stalled and 2 <= stalled[0] < 40
    # (a margin of one epoch either way: the kernels' objective and the oracle's differ in the last bits)
    model.fit(_frame())
    assert abs(len(model.loss_history) - (stalled[0] + 1)) <= 1
    assert abs(model.loss_history[-1] - model.loss_history[-2]) < 1e-5
    free = IALS(ials_config(reg=50.0, alpha=1.0, epochs=stalled[0] + 4, early_stop=False))
    free.fit(_frame())
    assert len(free.loss_history) == stalled[0] + 4


def test_model_argument_errors():
    import pandas as pd
    from daisyrec_amd.model import IALS
    for over in (dict(reg=0.0), dict(reg=-0.1), dict(alpha=-1.0)):
        with pytest.raises(ValueError):
            IALS(ials_config(**over))
    model = IALS(ials_config())
    good = dict(user=[0, 1], item=[2, 3], rating=[1.0, 2.0])
    for over in (dict(rating=[1.0, -2.0]), dict(rating=[1.0, float("nan")]), dict(rating=[float("inf"), 1.0]),
                 dict(user=[0, 40]), dict(item=[-1, 3]), dict(item=[2, 60])):
        with pytest.raises(ValueError):
            model.fit(pd.DataFrame(dict(good, **over)))
    for call in (lambda: model.predict(0, 0), lambda: model.full_rank(0), lambda: model.rank([]),
                 lambda: model.full_rank_users([0]), lambda: model.full_rank_positions([0], {0: {1}}),
                 lambda: model.fold_in({0: {1: 1.0}})):
        with pytest.raises(RuntimeError, match="fit"):
            call()


# ---- 7. fold-in --------------------------------------------------------------------------------------------------------------
def test_fold_in():
    from daisyrec_amd import ops
    model, _, _ = fitted()
    P, Q = model.embed_user.weight.data, model.embed_item.weight.data
    before = (P.clone(), Q.clone())
    row_ptr, col, val = model_csr()
    # the training rows of five users: the rows the user half-sweep gives them
    X_all, _ = ops.ials_half_sweep(_csr((row_ptr, col, val)), Q, ALPHA, REG)
    five = [0, 5, 17, 23, 39]                                    # (17 has no interactions)
    hist = {k: {int(col[e]): float(val[e]) for e in range(row_ptr[u], row_ptr[u + 1])} for k, u in enumerate(five)}
    hist.setdefault(4, {})
    X5 = model.fold_in(hist)
    assert X5.dtype == torch.float32 and tuple(X5.shape) == (5, 8)
    assert torch.equal(X5, X_all[five]) and not bool(X5[2].any())
    # histories that are in no training row, as a CSR triple
    rng = np.random.default_rng(12)
    new = O.csr_of_lengths([4, 0, 9, 1], 60, rng)
    Xn = model.fold_in(_csr(new))
    want = O.half_sweep(*new, _np(Q), ALPHA, REG)
    assert np.all(np.abs(_np(Xn).astype(np.float64) - want) <= _bound(want))
    ids = ops.full_rank_users(Xn, Q, torch.arange(4), 10, exclude=_csr(new)[:2])
    assert tuple(ids.shape) == (4, 10) and not np.isin(_np(ids)[0], new[1][:4]).any()
    with pytest.raises(IndexError):
        model.fold_in({0: {60: 1.0}})
    assert torch.equal(P, before[0]) and torch.equal(Q, before[1])
