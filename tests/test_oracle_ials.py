"""The iALS oracle (tests/ials_oracle.py) against a brute-force statement over all cells that shares none of its algebra,
the premises of the exact-solve construction the GPU test relies on, and the argument checks of the three entry points
of csrc/ials.hip, which precede every HIP call.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import ials_oracle as O

EXACT_DIMS = {8: 3, 24: 3, 64: 3, 100: 3, 128: 3}           # d -> the seed of exact_solve_fixture the GPU test uses


def small_case():
    rng = np.random.default_rng(5)
    U, I, d = 7, 9, 3
    row_ptr, col, val = O.csr_of_lengths([0, 1, 2, 3, 4, 9, 5], I, rng)
    X = rng.standard_normal((U, d))
    Y = rng.standard_normal((I, d))
    return U, I, d, row_ptr, col, val, X, Y


def dense(row_ptr, col, val, U, I, alpha):
    """preference and confidence of every cell"""
    p, c = np.zeros((U, I)), np.ones((U, I))
    for u in range(U):
        for e in range(row_ptr[u], row_ptr[u + 1]):
            p[u, col[e]] = 1.0
            c[u, col[e]] = 1.0 + alpha * val[e]
    return p, c


def brute_objective(p, c, X, Y, reg):
    total = 0.0
    for u in range(len(X)):
        for i in range(len(Y)):
            total += c[u, i] * (p[u, i] - float(np.dot(X[u], Y[i]))) ** 2
    return total + reg * (float((X ** 2).sum()) + float((Y ** 2).sum()))


@pytest.mark.parametrize("alpha,reg", [(10.0, 0.1), (0.5, 2.0), (0.0, 0.05)])
def test_objective_equals_the_sum_over_all_63_cells(alpha, reg):
    U, I, d, row_ptr, col, val, X, Y = small_case()
    p, c = dense(row_ptr, col, val, U, I, alpha)
    want = brute_objective(p, c, X, Y, reg)
    got = O.objective(row_ptr, col, val, X, Y, alpha, reg)
    assert abs(got - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("alpha,reg", [(10.0, 0.1), (0.5, 2.0), (40.0, 0.01)])
def test_the_gradient_vanishes_at_every_half_sweeps_solution(alpha, reg):
    """d/dx_u of the dense objective, -2 sum_i c_ui (p_ui - <x_u, y_i>) y_i + 2 reg x_u, at the fp64 solutions of the
    user half-sweep and then of the item half-sweep; relative to the size of its two cancelling parts"""
    U, I, d, row_ptr, col, val, X, Y = small_case()
    p, c = dense(row_ptr, col, val, U, I, alpha)
    Xs = O.half_sweep(row_ptr, col, val, Y, alpha, reg, round32=False)
    for u in range(U):
        if row_ptr[u + 1] == row_ptr[u]:
            assert not Xs[u].any()                               # an empty row: zeros (the minimiser: b = 0)
        parts = [-2 * c[u, i] * (p[u, i] - Xs[u] @ Y[i]) * Y[i] for i in range(I)] + [2 * reg * Xs[u]]
        scale = max(1.0, sum(np.abs(t).max() for t in parts))
        assert np.abs(sum(parts)).max() <= 1e-12 * scale, u
    t_ptr, t_col, t_val = O.transpose(row_ptr, col, val, I)
    Ys = O.half_sweep(t_ptr, t_col, t_val, Xs, alpha, reg, round32=False)
    for i in range(I):
        parts = [-2 * c[u, i] * (p[u, i] - Xs[u] @ Ys[i]) * Xs[u] for u in range(U)] + [2 * reg * Ys[i]]
        scale = max(1.0, sum(np.abs(t).max() for t in parts))
        assert np.abs(sum(parts)).max() <= 1e-12 * scale, i
    # and a full sweep does not raise the objective
    before = O.objective(row_ptr, col, val, X, Y, alpha, reg)
    mid = O.objective(row_ptr, col, val, Xs, Y, alpha, reg)
    after = O.objective(row_ptr, col, val, Xs, Ys, alpha, reg)
    assert after <= mid <= before


def test_transpose_matches_a_dense_transpose():
    U, I, d, row_ptr, col, val, X, Y = small_case()
    D = np.zeros((U, I))
    for u in range(U):
        D[u, col[row_ptr[u]:row_ptr[u + 1]]] = val[row_ptr[u]:row_ptr[u + 1]]
    t_ptr, t_col, t_val = O.transpose(row_ptr, col, val, I)
    T = np.zeros((I, U))
    for i in range(I):
        assert np.all(np.diff(t_col[t_ptr[i]:t_ptr[i + 1]]) > 0)
        T[i, t_col[t_ptr[i]:t_ptr[i + 1]]] = t_val[t_ptr[i]:t_ptr[i + 1]]
    assert np.array_equal(T, D.T)


def exact_case(d):
    """(L, the user rows as a CSR of random subsets with rating 1, the exact solutions as float64)"""
    L = O.exact_solve_fixture(d, EXACT_DIMS[d])
    rng = np.random.default_rng(100 + d)
    subsets = [np.sort(rng.choice(d, n, replace=False)) for n in (1, 2, max(1, d // 2), d, 3, max(1, d - 1))]
    row_ptr = np.zeros(len(subsets) + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum([len(s) for s in subsets])
    col = np.concatenate(subsets).astype(np.int32)
    sols, oks = zip(*(O.exact_solution(L, set(int(v) for v in s)) for s in subsets))
    want = np.array([[float(v) for v in x] for x in sols])
    return L, (row_ptr, col, np.ones(len(col), dtype=np.float32)), want, all(oks)


@pytest.mark.parametrize("d", sorted(EXACT_DIMS))
def test_the_exact_solve_fixtures_are_exact(d):
    """Y = L^T gives Y^T Y = L L^T in integers, its Cholesky factor is L itself, b = L 1_S, and x = L^-T 1_S is a
    dyadic vector every element of which - and every partial sum on the way - is exact in fp64 and fp32"""
    L, (row_ptr, col, val), want, ok = exact_case(d)
    assert ok
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    Y = L.T.copy()
    A, b = O.normal_equations(row_ptr, col, val, Y, 0.0, 0.0)
    assert np.array_equal(A[0], L @ L.T)
    assert np.array_equal(np.linalg.cholesky(A[0]), L)
    for u in range(len(want)):
        ind = np.zeros(d)
        ind[col[row_ptr[u]:row_ptr[u + 1]]] = 1.0
        assert np.array_equal(b[u], L @ ind)
        assert np.array_equal(A[u] @ want[u], b[u])              # zero residual, in exact arithmetic
    # the fit is perfect: the weights do not move the solution
    A2, b2 = O.normal_equations(row_ptr, col, val, Y, 3.0, 0.0)
    for u in range(len(want)):
        assert np.array_equal(A2[u] @ want[u], b2[u])


def test_not_every_such_factor_has_an_fp32_solution():
    """the representability check is a check: a factor of the same family - unit diagonal, -1 in the two columns before
    it - makes the back substitution a Fibonacci recurrence, whose values leave fp32's 24 bits after 36 rows"""
    d = 128
    L = np.eye(d)
    for i in range(1, d):
        L[i, max(0, i - 2):i] = -1.0
    x, ok = O.exact_solution(L, {d - 1})
    assert not ok and x[0] > 1 << 24
    x, ok = O.exact_solution(L[:30, :30], {29})
    assert ok and x[0] == 832040                                 # F(30)


def model_case():
    """U = 40, I = 60: the training frame of the model tests as arrays (some duplicate pairs, one user and a few items
    without interactions)"""
    rng = np.random.default_rng(11)
    U, I = 40, 60
    users = np.concatenate([np.full(n, u) for u, n in enumerate(rng.integers(1, 12, U)) if u != 17])
    items = rng.integers(0, I - 3, len(users))
    ratings = rng.integers(1, 6, len(users)).astype(np.float64)
    return U, I, users.astype(np.int64), items.astype(np.int64), ratings


def model_csr():
    U, I, users, items, ratings = model_case()
    D = np.zeros((U, I))
    np.add.at(D, (users, items), ratings)                        # duplicate pairs are summed
    row_ptr = np.zeros(U + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum((D != 0).sum(1))
    col = np.concatenate([np.nonzero(D[u])[0] for u in range(U)]).astype(np.int32)
    val = np.concatenate([D[u][D[u] != 0] for u in range(U)]).astype(np.float32)
    return row_ptr, col, val


def test_the_model_fixtures_objective_falls_strictly():
    U, I, *_ = model_case()
    row_ptr, col, val = model_csr()
    rng = np.random.default_rng(3)
    P0, Q0 = ((0.01 * rng.standard_normal((n, 8))).astype(np.float32) for n in (U, I))
    for round32 in (True, False):
        losses = O.fit(row_ptr, col, val, P0, Q0, 10.0, 0.1, 3, round32)[2]
        assert losses[0] > losses[1] > losses[2] and losses[1] - losses[2] > 1e-3


# ---- the entry points' argument checks -----------------------------------------------------------------------------------
def _gram(N, buf, **over):
    a = dict(Y=buf, n=10, ld=8, d=8, G=buf, ws=buf, ws_bytes=1 << 30)
    a.update(over)
    return N.lib.daisy_ials_gram(a["Y"], a["n"], a["ld"], a["d"], a["G"], a["ws"], a["ws_bytes"], None)


def _sweep(N, buf, **over):
    a = dict(rp=buf, col=buf, val=buf, rows=4, nnz=8, n=10, Y=buf, ldy=8, d=8, G=buf, alpha=1.0, reg=0.1, X=buf, ldx=8,
             info=buf, dA=None, db=None)
    a.update(over)
    return N.lib.daisy_ials_half_sweep(a["rp"], a["col"], a["val"], a["rows"], a["nnz"], a["n"], a["Y"], a["ldy"], a["d"], a["G"],
                                       a["alpha"], a["reg"], a["X"], a["ldx"], a["info"], a["dA"], a["db"], None)


def _objective(N, buf, **over):
    a = dict(rp=buf, col=buf, val=buf, rows=4, nnz=8, n=10, X=buf, ldx=8, Y=buf, ldy=8, d=8, G=buf, alpha=1.0, reg=0.1,
             out=buf, ws=buf, ws_bytes=1 << 30)
    a.update(over)
    return N.lib.daisy_ials_objective(a["rp"], a["col"], a["val"], a["rows"], a["nnz"], a["n"], a["X"], a["ldx"], a["Y"], a["ldy"],
                                      a["d"], a["G"], a["alpha"], a["reg"], a["out"], a["ws"], a["ws_bytes"], None)


def test_argument_errors_do_not_need_a_gpu():
    """every check precedes the first HIP call (the pointers are dummies nobody reads)"""
    from daisyrec_amd import _native as N
    buf = ctypes.create_string_buffer(256)
    d = ctypes.addressof(buf)
    nan, inf = float("nan"), float("inf")
    table = {
        "ials_gram": (_gram, [(dict(Y=None), "NULL"), (dict(G=None), "NULL"), (dict(ws=None), "NULL"), (dict(d=0), "d=0"),
                              (dict(d=129), "[1, 128]"), (dict(ld=7), "ld=7"), (dict(n=0), "n=0"), (dict(n=-1), "n=-1"),
                              (dict(ws_bytes=8), "workspace")]),
        "ials_half_sweep": (_sweep, [(dict(rp=None), "NULL"), (dict(col=None), "NULL"), (dict(val=None), "NULL"),
                                     (dict(Y=None), "NULL"), (dict(G=None), "NULL"), (dict(X=None), "NULL"),
                                     (dict(info=None), "NULL"), (dict(d=0), "d=0"), (dict(d=129), "[1, 128]"),
                                     (dict(ldy=7), "ldy=7"), (dict(ldx=7), "ldx=7"), (dict(rows=-1), "rows=-1"),
                                     (dict(nnz=-1), "nnz=-1"), (dict(n=0), "n_other=0"), (dict(alpha=nan), "alpha=nan"),
                                     (dict(alpha=inf), "alpha=inf"), (dict(reg=nan), "reg=nan"), (dict(reg=-inf), "reg=-inf")]),
        "ials_objective": (_objective, [(dict(rp=None), "NULL"), (dict(col=None), "NULL"), (dict(val=None), "NULL"),
                                        (dict(X=None), "NULL"), (dict(Y=None), "NULL"), (dict(G=None), "NULL"),
                                        (dict(out=None), "NULL"), (dict(ws=None), "NULL"), (dict(d=0), "d=0"),
                                        (dict(d=129), "[1, 128]"), (dict(ldy=7), "ldy=7"), (dict(ldx=7), "ldx=7"),
                                        (dict(rows=-1), "rows=-1"), (dict(n=0), "n_other=0"), (dict(alpha=nan), "alpha=nan"),
                                        (dict(reg=inf), "reg=inf"), (dict(ws_bytes=8), "workspace")]),
    }
    for name, (call, cases) in table.items():
        for over, text in cases:
            rc = call(N, d, **over)
            assert rc == N.DAISY_ERR_ARG, (name, over, rc)
            msg = N.last_error()
            assert msg.startswith(name + ":") and text in msg, (name, over, msg)
    with pytest.raises(ValueError, match="128"):
        N.check(_sweep(N, d, d=129))
    assert N.lib.daisy_ials_gram_workspace_bytes(0, 8) == 0 and N.lib.daisy_ials_gram_workspace_bytes(10, 129) == 0
    assert N.lib.daisy_ials_gram_workspace_bytes(10, 8) == 512          # one block's [8, 8] partial product
    assert N.lib.daisy_ials_objective_workspace_bytes(-1) == 0
    assert N.lib.daisy_ials_objective_workspace_bytes(1000) == 8192     # one partial per row, rounded up to 256 bytes
    assert N.IALS_MAX_D == 128


def test_the_model_checks_its_config_without_a_gpu():
    from conftest import mf_config
    from daisyrec_amd.model import IALS
    cfg = mf_config(user_num=5, item_num=6, factors=4, reg=0.1, alpha=1.0, epochs=1)
    for over in (dict(reg=0.0), dict(reg=-1.0), dict(reg=float("nan")), dict(alpha=-0.5), dict(alpha=float("inf")),
                 dict(factors=129), dict(factors=0), dict(topk=0), dict(user_num=0)):
        with pytest.raises(ValueError):
            IALS(dict(cfg, **over))
    model = IALS(cfg)
    assert tuple(model.embed_user.weight.shape) == (5, 4) and tuple(model.embed_item.weight.shape) == (6, 4)
    assert sorted(model.state_dict()) == ["embed_item.weight", "embed_user.weight"]
