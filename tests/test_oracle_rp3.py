"""The oracle of the two-hop walk (tests/rp3_oracle.py) against independent arithmetic, on the CPU: the dense fp64 product
on a case whose every sum is exact, and a scipy restatement of RP3beta on real-valued data within the bound of a float32
sum of positive terms."""
import numpy as np
import pytest

import rp3_oracle as O

U, I, K = O.U, O.I, 10
pattern, dyadic_case = O.pattern, O.dyadic_case


def boundary_ties(w_dense, K):
    """rows whose K-th and (K+1)-th largest positive weights are equal: the tie rule decides what is kept"""
    ties = 0
    for w in w_dense:
        pos = np.sort(w[w > 0])[::-1]
        ties += len(pos) > K and pos[K - 1] == pos[K]
    return ties


def test_dyadic_case_equals_the_dense_fp64_product_bit_for_bit():
    X, A, B, scale = dyadic_case()
    full = (O.dense_of(A, U) @ O.dense_of(B, I)) * scale.astype(np.float64)[None, :]      # fp64, exact
    np.fill_diagonal(full, 0.0)
    for i in (0, 7, I - 1):
        w = O.walk_row(A, B, i, I) * scale
        w[i] = 0
        assert w.dtype == np.float32 and np.array_equal(w.astype(np.float64), full[i])
    count, cols, vals = O.walk2_topk(A, B, I, K, scale)
    ties = boundary_ties(full, K)
    print(f"rows with a tie at the K = {K} boundary: {ties} of {I}")
    assert ties >= I // 4                                   # the tie rule is really exercised
    for i in range(I):
        order = np.lexsort((np.arange(I), -full[i]))
        want = np.sort([j for j in order[:K] if full[i, j] > 0])
        assert count[i] == len(want) and np.array_equal(cols[i, :count[i]], want)
        assert np.array_equal(vals[i, :count[i]].astype(np.float64), full[i, want])
        assert np.all(cols[i, count[i]:] == -1) and np.all(vals[i, count[i]:] == 0)


def test_selection_rules():
    w = np.array([0.5, np.nan, -1.0, 0.5, 0.0, 2.0, 0.5, -0.0], dtype=np.float32)
    assert O.select_row(w, 2).tolist() == [0, 5]            # the tie at 0.5 goes to the lower column
    assert O.select_row(w, 3).tolist() == [0, 3, 5]
    assert O.select_row(w, 8).tolist() == [0, 3, 5, 6]      # zero, negative and NaN are never kept
    assert O.select_row(np.zeros(4, dtype=np.float32), 2).tolist() == []


def test_normalize_divides_by_the_sequential_float32_sum():
    X, A, B, scale = dyadic_case(1)
    count, cols, vals = O.walk2_topk(A, B, I, K, scale)
    _, cols_n, vals_n = O.walk2_topk(A, B, I, K, scale, normalize=True)
    assert np.array_equal(cols, cols_n)
    for i in range(I):
        s = np.float32(0)
        for v in vals[i, :count[i]]:
            s = np.float32(s + v)
        assert np.array_equal(vals_n[i, :count[i]], (vals[i, :count[i]] / s).astype(np.float32))


@pytest.mark.parametrize("alpha,beta", [(0.7, 0.4), (1.0, 0.6), (0.5, 0.0)])
def test_against_a_scipy_restatement_of_rp3beta(alpha, beta):
    """W = P_iu^alpha P_ui^alpha diag(deg^-beta) by scipy in fp64, top-K per row.  The oracle's operands are the fp64
    ones rounded to float32 (2^-24 relative each), a product of two of them is rounded once more, a sum of n positive
    terms in float32 is within n * 2^-24 of the exact sum of those terms, and the column scale and its product add two
    more roundings: every weight is within (n + 5) * 2^-24 relative, n = the users of the source item (to first order;
    the bound below doubles it for the higher-order terms)."""
    import scipy.sparse as sp
    X = pattern(3).astype(np.float64)
    Xs = sp.csr_matrix(X)
    deg_u, deg_i = X.sum(1), X.sum(0)
    Pui = sp.diags(np.where(deg_u > 0, 1.0 / np.maximum(deg_u, 1), 0)) @ Xs
    Piu = sp.diags(np.where(deg_i > 0, 1.0 / np.maximum(deg_i, 1), 0)) @ Xs.T.tocsr()
    Pui.data, Piu.data = Pui.data ** alpha, Piu.data ** alpha
    pen = np.where(deg_i > 0, np.maximum(deg_i, 1) ** -beta, 0)
    want = np.asarray((Piu @ Pui @ sp.diags(pen)).todense())
    np.fill_diagonal(want, 0.0)

    Piu32, Pui32 = O.model_operands(X, alpha)
    _, _, col_scale = O.model_scales(X, alpha, beta)
    count, cols, vals = O.walk2_topk(Piu32, Pui32, I, K, col_scale)
    got = O.dense_rows(count, cols, vals, I)
    n_terms = deg_i.max()
    bound = 2 * (n_terms + 5) * 2.0 ** -24
    for i in range(I):
        kept = cols[i, :count[i]]
        assert count[i] == min(K, int((want[i] > 0).sum()))
        assert np.all(np.abs(got[i, kept] - want[i, kept]) <= bound * want[i, kept])
        # the kept set is a top-K set of the fp64 weights up to that bound: nothing left out beats a kept one by more
        rest = np.setdiff1d(np.arange(I), kept)
        if count[i] and len(rest):
            assert want[i, rest].max() <= want[i, kept].min() * (1 + 2 * bound)


def test_model_scales_and_scores():
    X = pattern(5, 40, 30, 0.2).astype(np.float64) * np.random.default_rng(6).integers(1, 6, (40, 30))
    us, it, cs = O.model_scales(X, 0.7, 0.4)
    assert us.dtype == np.float32 and np.allclose(us[X.sum(1) > 0], X.sum(1)[X.sum(1) > 0] ** -0.7, rtol=1e-7)
    assert np.allclose(cs[(X != 0).sum(0) > 0], (X != 0).sum(0)[(X != 0).sum(0) > 0] ** -0.4, rtol=1e-7)
    Piu, Pui = O.model_operands(X, 0.7)
    assert np.allclose(O.dense_of(Pui, 30), (X / X.sum(1, keepdims=True)) ** 0.7, rtol=1e-6)
    assert np.allclose(O.dense_of(Piu, 40), (X.T / X.sum(0)[:, None]) ** 0.7, rtol=1e-6)
    count, cols, vals = O.walk2_topk(Piu, Pui, 30, 5, cs)
    W = O.dense_rows(count, cols, vals, 30)
    assert np.allclose(O.scores(X, W), X @ W, rtol=1e-12, atol=0)
    assert O.top_ids(np.array([1.0, 3.0, 3.0, 0.5]), 2).tolist() == [1, 2]
