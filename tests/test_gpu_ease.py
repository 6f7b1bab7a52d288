"""EASE on the device (csrc/ease.hip) against exact integer constructions, numpy / LAPACK, the oracle
(tests/ease_oracle.py) and the reference's golden vectors: the blocked Cholesky factor and its info, the blocked inverse
(exact where the factor is an integer matrix with an integer inverse, bitwise symmetric, residual against LAPACK's), the
column scaling, the fp64 scores and top-k, and the model end to end through EASE.fit(DataFrame).  Every tolerance comes
from what LAPACK or the oracle achieve on the same input, never from the device's own result."""
import functools

import numpy as np
import pytest
import torch

import ease_oracle as O
from test_oracle_ease import TAGS, TOPK, case, ease_config, oracle_B

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 15, 16, 17, 63, 64, 65, 130, 257]      # below, at and above the MFMA tile (16) and the block (64); 4 blocks + 1


def _dev(a, dtype=torch.float64):
    return torch.as_tensor(np.array(a)).to(DEV, dtype)              # (a copy: the cached inputs are read-only)


# ---- potrf -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _int_factor(n):
    """an integer lower-triangular L0 [n, n]: entries in [-3, 3], diagonal in [1, 4]; A = L0 L0^T is exact in fp64, and so is
    every intermediate of a Cholesky factorisation of it, in any summation order (integers below 16 n)"""
    rng = np.random.RandomState(n)
    L0 = np.tril(rng.randint(-3, 4, (n, n)), -1).astype(np.float64)
    L0[np.arange(n), np.arange(n)] = rng.randint(1, 5, n)
    L0.setflags(write=False)
    return L0


@pytest.mark.parametrize("n", SIZES)
def test_potrf_is_exact_on_an_integer_factor(n):
    from daisyrec_amd import ops
    L0 = _int_factor(n)
    A = L0 @ L0.T
    L, info, _ = ops.ease_potrf(_dev(A))
    L = L.cpu().numpy()
    assert int(info.item()) == 0
    assert np.array_equal(np.tril(L), L0)
    assert np.array_equal(np.triu(L, 1), np.triu(A, 1))            # the strict upper triangle is left as it was


@pytest.mark.parametrize("col", [5, 130, 256])                      # the first, a middle and the last block of 257 columns
def test_potrf_reports_the_first_bad_pivot(col):
    from daisyrec_amd import ops
    L0 = _int_factor(257).copy()
    L0[col, col] = 0.0
    _, info, _ = ops.ease_potrf(_dev(L0 @ L0.T))
    assert int(info.item()) == col + 1


def test_potrf_reports_a_pivot_that_is_not_a_number():
    from daisyrec_amd import ops
    A = _int_factor(130) @ _int_factor(130).T
    A[70, 70] = np.nan
    _, info, _ = ops.ease_potrf(_dev(A))
    assert int(info.item()) == 71


# ---- potri -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _nilpotent_factor(n):
    """L0 = I + N with N an integer matrix that is non-zero only in rows >= ceil(n / 2) and columns < ceil(n / 2): N^2 = 0,
    so L0^-1 = I - N exactly"""
    h = (n + 1) // 2
    N = np.zeros((n, n))
    N[h:, :h] = np.random.RandomState(100 + n).randint(-3, 4, (n - h, h))
    N.setflags(write=False)
    return N


@pytest.mark.parametrize("n", SIZES)
def test_potri_is_exact_on_a_factor_with_an_integer_inverse(n):
    from daisyrec_amd import ops
    N = _nilpotent_factor(n)
    L0, T0 = np.eye(n) + N, np.eye(n) - N
    assert np.array_equal(L0 @ T0, np.eye(n))
    L, info, ws = ops.ease_potrf(_dev(L0 @ L0.T))
    assert int(info.item()) == 0 and np.array_equal(np.tril(L.cpu().numpy()), L0)
    P = ops.ease_potri(L, ws).cpu().numpy()
    assert np.array_equal(P, T0.T @ T0)
    assert np.array_equal(ops.ease_potri(L, ws, inplace=True).cpu().numpy(), T0.T @ T0)       # P in L's storage


@functools.lru_cache(None)
def _spd(n):
    M = np.random.RandomState(200 + n).standard_normal((n + 20, n))
    A = M.T @ M + np.eye(n)
    A = (A + A.T) / 2
    res = np.abs(A @ np.linalg.inv(A) - np.eye(n)).max()
    A.setflags(write=False)
    return A, res


@pytest.mark.parametrize("n", [65, 130, 257])
def test_potri_general_residual_and_symmetry(n):
    from daisyrec_amd import ops
    A, lapack = _spd(n)
    L, info, ws = ops.ease_potrf(_dev(A))
    assert int(info.item()) == 0
    Lh = np.tril(L.cpu().numpy())
    P1, P2 = ops.ease_potri(L, ws), ops.ease_potri(L, ws)
    assert torch.equal(P1, P2)
    P = P1.cpu().numpy()
    res = np.abs(A @ P - np.eye(n)).max()
    fac = np.abs(Lh @ Lh.T - A).max() / np.abs(A).max()
    print(f"n={n}: |A P - I|_max {res:.2e} (np.linalg.inv {lapack:.2e}: {res / lapack:.2f} x), |L L^T - A|_max / |A|_max {fac:.2e}")
    assert res <= 100 * lapack
    assert np.array_equal(P, P.T)


# ---- weights ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 17, 130])
def test_weights_scale_the_columns(n):
    from daisyrec_amd import ops
    A, _ = _spd(130)
    P = np.ascontiguousarray(np.linalg.inv(A)[:n, :n])
    want = -P / np.diag(P)
    np.fill_diagonal(want, 0.0)
    B = ops.ease_weights(_dev(P)).cpu().numpy()
    assert np.array_equal(B, want)
    assert not np.diag(B).any() and not np.signbit(np.diag(B)).any()
    Pd = _dev(P)
    out = ops.ease_weights(Pd, inplace=True)                     # B in P's storage
    assert out.data_ptr() == Pd.data_ptr() and np.array_equal(out.cpu().numpy(), want)


def test_system_widens_and_adds_reg():
    from daisyrec_amd import ops
    G = np.random.RandomState(0).randint(0, 1 << 20, (70, 70)).astype(np.float32)
    A = ops.ease_system(_dev(G, torch.float32), 0.5).cpu().numpy()
    assert A.dtype == np.float64 and np.array_equal(A, G.astype(np.float64) + 0.5 * np.eye(70))


# ---- rank ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _int_rank_case():
    """5 users x 700 items (more than one pass of the 256 threads), integer ratings and integer weights: exact scores with
    many exact ties; user 2 has no history"""
    rng = np.random.RandomState(1)
    U, I = 5, 700
    X = np.where(rng.rand(U, I) < 0.05, rng.randint(1, 6, (U, I)), 0).astype(np.float64)
    X[2] = 0
    W = rng.randint(-2, 3, (I, I)).astype(np.float64)
    X.setflags(write=False)
    W.setflags(write=False)
    return X, W


def _csr(X):
    from daisyrec_amd import ops
    u, i = np.nonzero(X)
    return ops.slim_csr(_dev(u, torch.int64), _dev(i, torch.int64), _dev(X[u, i]), X.shape[0], X.shape[1])


def test_rank_ties_clamping_and_full_rank():
    from daisyrec_amd import ops
    X, W = _int_rank_case()
    U, I = X.shape
    full = X @ W
    csr, Wd, users = _csr(X), _dev(W), _dev(np.arange(U), torch.int64)
    sc, ids = ops.ease_rank(csr, Wd, users, None, 50)
    assert sc.dtype == torch.float64 and np.array_equal(sc.cpu().numpy(), full)
    assert np.array_equal(ids.cpu().numpy(), np.argsort(-full, axis=1, kind="stable")[:, :50])
    assert np.array_equal(ids.cpu().numpy()[2], np.arange(50))                       # no history: all 0, the first topk
    rng = np.random.RandomState(2)
    cands = np.stack([rng.permutation(I)[:7] for _ in range(U)]).astype(np.int64)
    sc, ids = ops.ease_rank(csr, Wd, users, _dev(cands, torch.int64), 10)            # topk > C: clamped
    assert ids.shape == (U, 7)
    assert np.array_equal(ids.cpu().numpy(), O.rank_lists(np.take_along_axis(full, cands, 1), cands, 7))
    sc, ids = ops.ease_rank(csr, Wd, users, _dev(cands, torch.int64), 0)             # scores only
    assert ids is None and np.array_equal(sc.cpu().numpy(), np.take_along_axis(full, cands, 1))


def test_rank_scores_zero_for_ids_out_of_range():
    from daisyrec_amd import ops
    X, W = _int_rank_case()
    U, I = X.shape
    full = X @ W
    csr, Wd = _csr(X), _dev(W)
    cands = np.array([[3, -1, I, 5], [I + 7, 0, 1, -9]], dtype=np.int64)
    sc, ids = ops.ease_rank(csr, Wd, _dev([0, 1], torch.int64), _dev(cands, torch.int64), 2)
    want = np.array([[full[0, 3], 0, 0, full[0, 5]], [0, full[1, 0], full[1, 1], 0]])
    assert np.array_equal(sc.cpu().numpy(), want)
    assert np.array_equal(ids.cpu().numpy(), O.rank_lists(want, cands, 2))
    sc, _ = ops.ease_rank(csr, Wd, _dev([U, -1, 0], torch.int64), _dev(np.tile([3, 5], (3, 1)), torch.int64))
    assert np.array_equal(sc.cpu().numpy(), [[0, 0], [0, 0], [full[0, 3], full[0, 5]]])


def test_rank_orders_on_the_fp64_keys():
    from daisyrec_amd import ops
    I = 40
    perm = np.random.RandomState(0).permutation(I)
    W = np.zeros((I, I))
    W[0] = 1.0 + perm * 1e-12                                   # all equal in fp32, distinct in fp64
    assert len(np.unique(W[0].astype(np.float32))) == 1 and len(np.unique(W[0])) == I
    X = np.zeros((1, I))
    X[0, 0] = 1.0
    sc, ids = ops.ease_rank(_csr(X), _dev(W), _dev([0], torch.int64), None, 10)
    assert np.array_equal(sc.cpu().numpy()[0], W[0]) and np.array_equal(ids.cpu().numpy()[0], np.argsort(-W[0], kind="stable")[:10])


# ---- the model end to end ------------------------------------------------------------------------------------------------------
def _frame(c):
    import pandas as pd
    return pd.DataFrame({"user": c["u"], "item": c["i"], "rating": c["r"]})


def _fit(tag):
    from daisyrec_amd.model import EASE
    c = case(tag)
    m = EASE(ease_config(user_num=c["U"], item_num=c["I"], reg=c["reg"], topk=TOPK))
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
def test_model_matches_the_reference(tag):
    c, m = case(tag), fitted(tag)
    assert m.fit_info["info"] == 0 and m.fit_info["bytes_held"] >= c["I"] * c["I"] * 8
    B = m.item_similarity
    assert isinstance(B, np.ndarray) and B.dtype == np.float64 and B.shape == (c["I"], c["I"]) and not np.diag(B).any()
    rows = c["B"].shape[0]
    bdev = np.abs(B[:rows] - c["B"]).max()
    sc = m._rank(np.arange(c["U"]), np.array(c["cands"]))[0].cpu().numpy()
    dev = np.abs(sc - c["scores_ref"]).max()
    print(f"{tag}: max |B - reference| {bdev:.2e} = {bdev / (c['B_tol'] / 100):.2f} x oracle_B_dev, max |score - reference| "
          f"{dev:.2e} = {dev / (c['tol'] / 100):.2f} x oracle_dev (allowed: 100 each)")
    assert bdev <= c["B_tol"]
    assert dev <= c["tol"]
    ranks = m.rank(_loader(c))
    assert ranks.dtype == np.int64 and ranks.shape == (c["U"], TOPK)
    assert np.array_equal(ranks[c["ranked"]], c["rank_ref"][c["ranked"]])
    # the user without history ('dup'): exactly 0 everywhere, the first topk candidates
    assert not sc[~c["ranked"]].any()
    assert np.array_equal(ranks[~c["ranked"]], c["cands"][~c["ranked"]][:, :TOPK])
    X = m.interaction_matrix
    import scipy.sparse as sp
    assert sp.isspmatrix_csr(X) and X.dtype == np.float32 and X.shape == (c["U"], c["I"])
    assert np.array_equal(np.asarray(X.todense(), dtype=np.float64), c["X"])


@pytest.mark.parametrize("tag", TAGS)
def test_full_rank_and_predict_agree_with_the_oracle(tag):
    c, m = case(tag), fitted(tag)
    want = c["X"] @ oracle_B(tag)
    top = -np.sort(-want, axis=1)[:, :TOPK + 1]
    assert (top[:, :-1] - top[:, 1:])[c["ranked"]].min() >= 1e4 * c["tol"]       # the oracle's order is decided
    full, ids = m._rank(np.arange(c["U"]), None, TOPK)
    full, ids = full.cpu().numpy(), ids.cpu().numpy()
    assert np.abs(full - want).max() <= c["tol"]
    assert np.array_equal(ids[c["ranked"]], np.argsort(-want, axis=1, kind="stable")[:, :TOPK][c["ranked"]])
    assert np.array_equal(ids[~c["ranked"]], np.tile(np.arange(TOPK), ((~c["ranked"]).sum(), 1)))
    for u in (0, c["U"] // 2, c["U"] - 1):
        got = m.full_rank(u)
        assert got.dtype == np.int64 and got.shape == (TOPK,) and np.array_equal(got, ids[u])
        for i in (0, int(c["cands"][u, 0])):
            p = m.predict(u, i)
            assert isinstance(p, float) and p == full[u, i]
    with pytest.raises(IndexError):
        m.predict(c["U"], 0)
    with pytest.raises(IndexError):
        m.predict(0, c["I"])


@pytest.mark.parametrize("tag", ["blocks", "wide"])
def test_second_fit_is_bitwise_identical(tag):
    a, b = fitted(tag), _fit(tag)
    assert torch.equal(a._B, b._B)


def test_fit_refuses_an_offer_that_is_too_small():
    from daisyrec_amd import _native as N, ops
    c = case("blocks")
    csr = ops.slim_csr(_dev(c["u"], torch.int64), _dev(c["i"], torch.int64), _dev(c["r"]), c["U"], c["I"])
    need = N.lib.daisy_ease_fit_bytes(c["I"])
    with pytest.raises(ValueError, match="does not fit"):
        ops.ease_fit(csr, c["I"], c["reg"], offered_bytes=need - 1)
    B, info = ops.ease_fit(csr, c["I"], c["reg"], offered_bytes=need + (4 << 20))
    assert int(info.item()) == 0 and torch.equal(B, fitted("blocks")._B)


def test_calls_before_fit_are_refused():
    from daisyrec_amd.model import EASE
    m = EASE(ease_config())
    with pytest.raises(RuntimeError, match="fit"):
        m.full_rank(0)
    with pytest.raises(RuntimeError, match="fit"):
        m.predict(0, 0)
