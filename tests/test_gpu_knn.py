"""ItemKNN / UserKNN on the device (csrc/knn.hip): the radix select against the oracle's selection on constructed weights
(exact: the same fp32 operations, the same tie rule), the means and the centring on data whose means are dyadic, the fp64
score kernel on exact integer cases in both operand roles, and the models end to end against the reference's golden
vectors under each fixture's regime (tests/knn_oracle.py).  Every tolerance is the one tests/golden/make_golden_knn.py
measured for the oracle, or the fp64 bound of a sum taken in another order; none comes from the device's result."""
import functools

import numpy as np
import pytest
import torch

import knn_oracle as O
from test_oracle_knn import SCORED, TAGS, TOPK, case, check_scores, check_W, knn_config, oracle_W

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a)).to(DEV, dtype)


def _select(G, ss, mode, shrink, K):
    from daisyrec_amd import ops
    out = ops.knn_select(_dev(G), _dev(ss), mode, shrink, K)
    return tuple(t.cpu().numpy() for t in out)


def _same_selection(G, ss, mode, shrink, K):
    want = O.select(O.weights(G, ss, mode, shrink), K)
    got = _select(G, ss, mode, shrink, K)
    for name, g, w in zip(("count", "rows", "vals"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g.view(np.uint32) if name == "vals" else g, w.view(np.uint32) if name == "vals" else w), name
    return got


# ---- select ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 45, 255, 256, 257, 700])
def test_select_integer_weights_with_many_ties(n):
    rng = np.random.RandomState(n)
    G = np.where(rng.rand(n, n) < 0.4, rng.randint(1, 6, (n, n)), 0).astype(F32)
    ss = np.ones(n, dtype=F32)
    for K in sorted({1, 7, n - 1, n, n + 5} - {0}):
        count, rows, _ = _same_selection(G, ss, "plain", 0, K)
        assert count.max() <= min(K, n) and not np.any(rows == np.arange(n)[:, None])       # never the column itself


@pytest.mark.parametrize("base", [20, 23])
@pytest.mark.parametrize("K", [1, 7, 40, 255, 300])
def test_select_keys_that_differ_in_the_lowest_digit_only(K, base):
    """2^23 + perm: ulp 1, the 256 keys of a row differ in the low 8 bits alone; 2^20 + perm: ulp 1/8, bits 3 .. 10, so
    the last two passes both decide"""
    n = 256
    rng = np.random.RandomState(K)
    G = (2.0 ** base + np.stack([rng.permutation(n) for _ in range(n)])).astype(F32)
    assert len(np.unique(G[0])) == n and len(np.unique(G[0].view(np.uint32) >> (8 if base == 23 else 16))) == 1
    _same_selection(G, np.ones(n, dtype=F32), "plain", 0, K)


def test_select_signs_zeros_and_empty_rows():
    n = 300
    rng = np.random.RandomState(0)
    G = -rng.randint(1, 9, (n, n)).astype(F32)                     # all negative ...
    for j in range(n):
        pos = rng.permutation(n)[:12]
        G[j, pos[:5]] = rng.randint(1, 4, 5)                       # ... but 5 positives (with ties)
        G[j, pos[5:9]] = 0.0                                       # and 4 + 3 zeros of either sign
        G[j, pos[9:]] = -0.0
    G[17] = 0.0                                                     # an all-zero row
    G[18] = -0.0
    assert np.signbit(G[0]).sum() > 250 and (G[0] == 0).sum() >= 6
    ss = np.ones(n, dtype=F32)
    for K in (3, 5, 8, 12, 13, 40):                                 # inside the positives, inside the zeros, into the negatives
        count, rows, vals = _same_selection(G, ss, "plain", 0, K)
        assert count[17] == 0 and count[18] == 0 and not (vals == 0)[rows >= 0].any()
    assert count[0] > 5 and (vals[0] < 0).sum() == count[0] - 5     # K = 40: zeros outrank the negatives and are dropped


@pytest.mark.parametrize("mode,shrink", [("cosine", 10.0), ("cosine", 0.0), ("tanimoto", 0.0), ("dice", 0.5), ("tversky", 0.0),
                                         ("plain", 10.0), ("plain", 0.0)])
def test_select_weight_arithmetic_is_the_reference_fp32_sequence(mode, shrink):
    n = 300
    rng = np.random.RandomState(1)
    A = rng.standard_normal((n, n)).astype(F32)
    G = (A + A.T).astype(F32)
    ss = (1.0 + 3.0 * rng.rand(n)).astype(F32)
    _same_selection(G, ss, mode, shrink, 40)


def test_select_k_1024_of_1500():
    n = 1500
    rng = np.random.RandomState(2)
    G = rng.standard_normal((n, n)).astype(F32)
    ss = (1.0 + rng.rand(n)).astype(F32)
    count, _, _ = _same_selection(G, ss, "cosine", 100.0, 1024)
    assert count.min() >= 1023 and count.max() <= 1024         # (the column's own zero is among the 1024 largest, and dropped)
    a, b = _select(G, ss, "cosine", 100.0, 1024), _select(G, ss, "cosine", 100.0, 1024)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_select_asymmetric_half_is_cosine_and_diag():
    from daisyrec_amd import ops
    n = 130
    rng = np.random.RandomState(3)
    A = rng.randint(0, 4, (200, n)).astype(F32)
    G = (A.T @ A).astype(F32)
    ss = ops.knn_diag(_dev(G), True).cpu().numpy()
    assert np.array_equal(ss, np.sqrt(np.diag(G))) and np.array_equal(ops.knn_diag(_dev(G), False).cpu().numpy(), np.diag(G))
    a = _select(G, ss, "asymmetric", 100.0, 7)
    b = _same_selection(G, ss, "cosine", 100.0, 7)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- means and centring --------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _dyadic():
    """A [60, 300] whose rows hold 0, 1, 2, 4, ... 256 integer entries: every mean is exact"""
    rng = np.random.RandomState(4)
    R, Cn = 60, 300
    M = np.zeros((R, Cn), dtype=bool)
    for r in range(R):
        cnt = [0, 1, 2, 4, 8, 16, 64, 128, 256][r % 9]
        M[r, rng.permutation(Cn)[:cnt]] = True
    A = np.where(M, rng.randint(1, 6, (R, Cn)), 0).astype(np.float64)
    A.setflags(write=False)
    M.setflags(write=False)
    return A, M


def _csr_of(A, M):
    from daisyrec_amd import ops
    r, c = np.nonzero(M)
    return ops.slim_csr(_dev(r, torch.int64), _dev(c, torch.int64), _dev(A[r, c], torch.float64), A.shape[0], A.shape[1])


def _csr_dense(csr, shape):
    ptr, col, val = (t.cpu().numpy() for t in csr)
    out = np.zeros(shape, dtype=F32)
    for r in range(shape[0]):
        out[r, col[ptr[r]:ptr[r + 1]]] = val[ptr[r]:ptr[r + 1]]
    return out


def test_means_and_centring_are_exact_on_dyadic_data():
    from daisyrec_amd import ops
    A, M = _dyadic()
    csr, csr_t = _csr_of(A, M), _csr_of(A.T, M.T)
    mean = ops.knn_row_means(csr)
    want = O.row_means(A.astype(F32), M)
    assert np.array_equal(mean.cpu().numpy(), want) and not want[~M.any(1)].any() and (~M.any(1)).sum() >= 6
    assert len(np.unique(want)) > 10 and np.any(want != np.round(want))
    assert np.array_equal(_csr_dense(ops.knn_center(csr, A.shape[1], "row", mean), A.shape), O.prepare(A, M, "adjusted"))
    # the column means of A^T are the row means of A
    assert np.array_equal(_csr_dense(ops.knn_center(csr_t, A.shape[0], "col", mean), A.T.shape), O.prepare(A.T, M.T, "pearson"))
    assert np.array_equal(_csr_dense(ops.knn_center(csr, A.shape[1], "binary"), A.shape), M.astype(F32))
    assert np.array_equal(_csr_dense(ops.knn_center(csr, A.shape[1], "none"), A.shape), A.astype(F32))
    centred = ops.knn_center(csr, A.shape[1], "row", mean)
    assert centred[2].numel() == csr[2].numel() and (centred[2] == 0).any()      # a value centred to exactly 0 stays stored


# ---- rank ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _int_rank_case():
    """5 users x 700 items (more than one pass of the 256 threads), integer ratings; W [700, 700] sparse integers for the
    ItemKNN role, S [5, 5] integers for the UserKNN role: exact scores with many exact ties; user 2 has no history and
    row 2 of S is empty"""
    rng = np.random.RandomState(1)
    U, I = 5, 700
    X = np.where(rng.rand(U, I) < 0.05, rng.randint(1, 6, (U, I)), 0).astype(np.float64)
    X[2] = 0
    W = np.where(rng.rand(I, I) < 0.05, rng.randint(-2, 3, (I, I)), 0).astype(np.float64)
    S = rng.randint(-2, 3, (U, U)).astype(np.float64)
    S[2] = 0
    for a in (X, W, S):
        a.setflags(write=False)
    return X, W, S


def _triple(A, by_column=False):
    """the CSR of A (by_column: of A^T, i.e. A by column) with the stored entries = the non-zeros"""
    A = A.T if by_column else A
    return _csr_of(A, A != 0)


@pytest.mark.parametrize("role", ["item", "user"])
@pytest.mark.parametrize("path", ["lds", "global"])
def test_rank_exact_integer_case(role, path):
    from daisyrec_amd import ops
    X, W, S = _int_rank_case()
    U, I = X.shape
    if role == "item":
        full, L, R, inner = X @ W, _triple(X), _triple(W, True), I
    else:
        full, L, R, inner = S @ X, _triple(S), _triple(X, True), U
    users = _dev(np.arange(U), torch.int64)
    sc, ids = ops.knn_rank(L, R, inner, I, users, None, 50, path=path)
    assert sc.dtype == torch.float64 and np.array_equal(sc.cpu().numpy(), full)
    assert ids.dtype == torch.int64 and np.array_equal(ids.cpu().numpy(), np.argsort(-full, axis=1, kind="stable")[:, :50])
    assert np.array_equal(ids.cpu().numpy()[2], np.arange(50))                       # nothing to sum: all 0, the first topk
    rng = np.random.RandomState(2)
    cands = np.stack([rng.permutation(I)[:7] for _ in range(U)]).astype(np.int64)
    sc, ids = ops.knn_rank(L, R, inner, I, users, _dev(cands, torch.int64), 10, path=path)      # topk > C: clamped
    assert ids.shape == (U, 7)
    assert np.array_equal(ids.cpu().numpy(), O.rank_lists(np.take_along_axis(full, cands, 1), cands, 7))
    sc, ids = ops.knn_rank(L, R, inner, I, users, _dev(cands, torch.int64), 0, path=path)       # scores only
    assert ids is None and np.array_equal(sc.cpu().numpy(), np.take_along_axis(full, cands, 1))
    # ids out of range score 0
    cands = np.array([[3, -1, I, 5], [I + 7, 0, 1, -9]], dtype=np.int64)
    sc, ids = ops.knn_rank(L, R, inner, I, _dev([0, 1], torch.int64), _dev(cands, torch.int64), 2, path=path)
    want = np.array([[full[0, 3], 0, 0, full[0, 5]], [0, full[1, 0], full[1, 1], 0]])
    assert np.array_equal(sc.cpu().numpy(), want) and np.array_equal(ids.cpu().numpy(), O.rank_lists(want, cands, 2))
    sc, _ = ops.knn_rank(L, R, inner, I, _dev([U, -1, 0], torch.int64), _dev(np.tile([3, 5], (3, 1)), torch.int64), path=path)
    assert np.array_equal(sc.cpu().numpy(), [[0, 0], [0, 0], [full[0, 3], full[0, 5]]])


def test_rank_orders_on_the_fp64_keys():
    from daisyrec_amd import ops
    I = 40
    perm = np.random.RandomState(0).permutation(I).astype(np.float64)
    Lm = np.array([[1.0, 2.0 ** -30]])
    Rm = np.stack([np.ones(I), perm])                        # score c = 1 + perm[c] 2^-30: equal in fp32, distinct in fp64
    Rm[1, perm == 0] = 0.0
    full = Lm @ Rm
    assert len(np.unique(full.astype(F32))) == 1 and len(np.unique(full)) == I
    R = _csr_of(Rm.T, np.ones((I, 2), dtype=bool))
    sc, ids = ops.knn_rank(_triple(Lm), R, 2, I, _dev([0], torch.int64), None, 10)
    assert np.array_equal(sc.cpu().numpy(), full) and np.array_equal(ids.cpu().numpy()[0], np.argsort(-full[0], kind="stable")[:10])


# ---- the models end to end -------------------------------------------------------------------------------------------------------
def _frame(c):
    import pandas as pd
    return pd.DataFrame({"user": c["u"], "item": c["i"], "rating": c["r"]})


def _fit(tag):
    from daisyrec_amd.model import ItemKNNCF, UserKNNCF
    c = case(tag)
    cls = ItemKNNCF if c["model"] == "item" else UserKNNCF
    m = cls(knn_config(user_num=c["U"], item_num=c["I"], maxk=c["K"], shrink=c["shrink"], normalize=c["normalize"],
                       similarity=c["sim"], topk=TOPK))
    m.fit(_frame(c))
    return m


@functools.lru_cache(None)
def fitted(tag):
    return _fit(tag)


def _loader(c, batch=64):
    users = np.arange(c["U"])
    return [(torch.from_numpy(users[b:b + batch]), torch.from_numpy(np.array(c["cands"][b:b + batch])))
            for b in range(0, c["U"], batch)]


@pytest.mark.parametrize("tag", TAGS)
def test_model_W_matches_the_reference(tag):
    import scipy.sparse as sp
    c, m = case(tag), fitted(tag)
    W = m.w_sparse
    assert sp.isspmatrix_csc(W) and W.dtype == np.float32 and W.shape == (c["n"], c["n"])
    assert m.fit_info["nnz"] == W.nnz and m.fit_info["n"] == c["n"] and m.fit_info["bytes_peak"] >= c["n"] * c["n"] * 4
    assert m.fit_info["bytes_held"] >= W.nnz * 8
    check_W(c, np.asarray(W.todense()), against_oracle=oracle_W(tag))


@pytest.mark.parametrize("tag", SCORED)
def test_model_scores_and_lists_match_the_reference(tag):
    c, m = case(tag), fitted(tag)
    sc = m._rank(np.arange(c["U"]), np.array(c["cands"]))[0].cpu().numpy()
    ranks = m.rank(_loader(c))
    assert ranks.dtype == np.int64
    check_scores(c, sc, ranks)
    # full_rank and predict read the same scores
    full, ids = m._rank(np.arange(c["U"]), None, TOPK)
    full, ids = full.cpu().numpy(), ids.cpu().numpy()
    assert np.array_equal(np.take_along_axis(full, c["cands"], 1), sc)
    assert np.array_equal(ids, np.argsort(-full, axis=1, kind="stable")[:, :TOPK])
    for u in (0, c["U"] // 2, c["U"] - 1):
        got = m.full_rank(u)
        assert got.dtype == np.int64 and got.shape == (min(TOPK, c["I"]),) and np.array_equal(got, ids[u])
        for i in (0, int(c["cands"][u, 0])):
            p = m.predict(u, i)
            assert isinstance(p, float) and p == full[u, i]
    with pytest.raises(IndexError):
        m.predict(c["U"], 0)
    with pytest.raises(IndexError):
        m.predict(0, c["I"])


@pytest.mark.parametrize("tag", ["cos45", "user"])
def test_pred_mat_is_the_scipy_matrix(tag):
    import scipy.sparse as sp
    c, m = case(tag), fitted(tag)
    P = m.pred_mat
    assert sp.issparse(P) and P.format == "lil" and P.dtype == np.float64 and P.shape == (c["U"], c["I"])
    assert np.array_equal(np.take_along_axis(np.asarray(P.todense()), c["cands"], 1),
                          m._rank(np.arange(c["U"]), np.array(c["cands"]))[0].cpu().numpy())


@pytest.mark.parametrize("tag", ["wide700", "user", "adjusted", "jaccard"])
def test_second_fit_is_bitwise_identical(tag):
    a, b = fitted(tag), _fit(tag)
    assert all(torch.equal(x, y) for x, y in zip(a._W, b._W))
    c = case(tag)
    users = np.arange(c["U"])
    assert torch.equal(a._rank(users, None, 0)[0], b._rank(users, None, 0)[0])


def test_fit_refuses_an_offer_that_is_too_small():
    from daisyrec_amd import _native as N, ops
    c = case("cos257")
    csr = ops.slim_csr(_dev(c["u"], torch.int64), _dev(c["i"], torch.int64), _dev(c["r"], torch.float64), c["U"], c["I"])
    need = N.lib.daisy_knn_fit_bytes(c["U"], c["I"], c["K"])
    with pytest.raises(ValueError, match="does not fit"):
        ops.knn_fit(csr, c["I"], c["sim"], c["shrink"], c["K"], offered_bytes=need - 1)
    W = ops.knn_fit(csr, c["I"], c["sim"], c["shrink"], c["K"], offered_bytes=need)
    assert all(torch.equal(x, y) for x, y in zip(W, fitted("cos257")._W))


def test_calls_before_fit_are_refused():
    from daisyrec_amd.model import ItemKNNCF, UserKNNCF
    for cls in (ItemKNNCF, UserKNNCF):
        m = cls(knn_config())
        assert m.pred_mat is None and m.w_sparse is None and m.fit_info is None
        with pytest.raises(RuntimeError, match="fit"):
            m.full_rank(0)
        with pytest.raises(RuntimeError, match="fit"):
            m.predict(0, 0)
        with pytest.raises(RuntimeError, match="fit"):
            m.rank([])
