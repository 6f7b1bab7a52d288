"""PureSVD on the device (csrc/puresvd.hip) against numpy / LAPACK, the oracle (tests/puresvd_oracle.py) and the reference's
golden vectors: the sparse product, the Gram matrix and the dense product on the fp64 MFMA (exact with small integers,
bitwise repeatable), the Cholesky factor with dropped columns, Cholesky-QR2, the Jacobi SVD, the fp64 top-k, and the model
end to end through PureSVD.fit(DataFrame).  Every tolerance is derived from what LAPACK / the QR oracle achieve on the
same input, never from the device's own result."""
import functools

import numpy as np
import pytest
import scipy.linalg
import torch

import puresvd_oracle as O
from test_oracle_puresvd import RANKED, TAGS, TOPK, case, oracle_fit, puresvd_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = O.EPS


def _dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype)


# ---- spmm --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _sparse_case():
    """40 x 400 with empty rows (0, 7, 39), one row of 300 non-zeros (> one workgroup's 256 threads) and integer values"""
    rng = np.random.RandomState(11)
    n, m = 40, 400
    A = np.zeros((n, m))
    for r in range(n):
        nnz = 300 if r == 3 else rng.randint(1, 20)
        A[r, rng.permutation(m)[:nnz]] = rng.randint(1, 6, nnz)
    A[[0, 7, 39]] = 0
    A.setflags(write=False)
    return A


@pytest.mark.parametrize("c", [1, 18, 160])
def test_spmm_is_exact_with_integers_and_repeatable(c):
    from daisyrec_amd import ops
    A = _sparse_case()
    n, m = A.shape
    u, i = np.nonzero(A)
    csr = ops.slim_csr(_dev(u, torch.int64), _dev(i, torch.int64), _dev(A[u, i]), n, m)
    X = np.random.RandomState(c).randint(-8, 9, (m, c)).astype(np.float64)
    Y1, Y2 = ops.psvd_spmm(csr, m, _dev(X)), ops.psvd_spmm(csr, m, _dev(X))
    assert Y1.dtype == torch.float64 and np.array_equal(Y1.cpu().numpy(), A @ X)
    assert not Y1.cpu().numpy()[[0, 7, 39]].any()
    assert torch.equal(Y1, Y2)


# ---- Gram and the dense product ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [18, 26, 160, 256])
@pytest.mark.parametrize("n", [1, 63, 1000])
def test_gram_is_exact_with_integers_and_repeatable(n, c):
    from daisyrec_amd import _native as N, ops
    Y = np.random.RandomState(n + c).randint(-4, 5, (n, c)).astype(np.float64)
    want = Y.T @ Y                                             # |entries| <= 16 n: exact
    default_rows = N.lib.daisy_psvd_gram_block_rows(n, 0)
    assert n < 1000 or -(-n // default_rows) >= 3               # n = 1000 spans at least 3 row blocks
    Yd = _dev(Y)
    for rows in (0, 100):                                      # the default block and 100 rows (10 blocks at n = 1000)
        G1, G2 = ops.psvd_gram(Yd, rows), ops.psvd_gram(Yd, rows)
        assert np.array_equal(G1.cpu().numpy(), want), f"block_rows={rows}"
        assert torch.equal(G1, G2)


@pytest.mark.parametrize("n,c,c2", [(1, 18, 18), (63, 26, 18), (100, 160, 160), (37, 256, 7), (256, 256, 256)])
def test_gemm_is_exact_with_integers(n, c, c2):
    from daisyrec_amd import ops
    rng = np.random.RandomState(n + c + c2)
    Y, T = rng.randint(-4, 5, (n, c)).astype(np.float64), rng.randint(-4, 5, (c, c2)).astype(np.float64)
    assert np.array_equal(ops.psvd_gemm(_dev(Y), _dev(T)).cpu().numpy(), Y @ T)


# ---- Cholesky and Cholesky-QR2 ----------------------------------------------------------------------------------------------
def test_chol_matches_the_literal_rule():
    from daisyrec_amd import ops
    rng = np.random.RandomState(3)
    Y = rng.standard_normal((200, 26))
    Y[:, 9] = Y[:, 1] + Y[:, 4]
    Y[:, 20] = 0.0
    G = Y.T @ Y
    R0, Ri0, d0 = O.chol_drop(G, 200)
    R, Ri, d = ops.psvd_chol(_dev(G), 200)
    R, Ri = R.cpu().numpy(), Ri.cpu().numpy()
    assert int(d.item()) == d0 == 2
    for M in (R, Ri):
        assert not M[9].any() and not M[20].any() and not np.tril(M, -1).any()
    assert R[:9, 9].any() and not Ri[:, 9].any() and not Ri[:, 20].any()
    # the factor of a matrix of condition kappa(Y)^2 ~ 1e2: a backward-stable result lies within c eps kappa^2 |R|
    scale = 26 * EPS * np.linalg.cond(np.delete(Y, [9, 20], axis=1)) ** 2
    assert np.abs(R - R0).max() <= scale * np.abs(R0).max()
    assert np.abs(Ri - Ri0).max() <= scale * np.abs(Ri0).max()


@functools.lru_cache(None)
def _orth_inputs():
    rng = np.random.RandomState(5)
    full = rng.standard_normal((500, 26))
    dep = full.copy()
    dep[:, 5] = dep[:, 0] - 2 * dep[:, 3]
    dep[:, 19] = dep[:, 7] + dep[:, 5] + 0.5 * dep[:, 18]
    low = rng.standard_normal((40, 12)) @ rng.standard_normal((12, 26))
    Q, R = scipy.linalg.qr(full, mode="economic")
    lapack = (np.abs(Q.T @ Q - np.eye(26)).max(), np.abs(Q @ R - full).max() / np.abs(full).max())
    return {"full": (full, []), "dependent": (dep, [5, 19]), "rank12": (low, list(range(12, 26)))}, lapack


@pytest.mark.parametrize("name", ["full", "dependent", "rank12"])
def test_orthonormalize(name):
    from daisyrec_amd import ops
    inputs, (lapack_orth, lapack_res) = _orth_inputs()
    Y, drop = inputs[name]
    n = Y.shape[0]
    Q, R, dropped = ops.psvd_orthonormalize(_dev(Y))
    Q, R = Q.cpu().numpy(), R.cpu().numpy()
    assert int(dropped.item()) == len(drop)
    assert not Q[:, drop].any() and not R[drop].any()          # exactly zero
    I_kept = np.eye(26)
    I_kept[drop, drop] = 0.0
    orth = np.abs(Q.T @ Q - I_kept).max()
    res = np.abs(Q @ R - Y).max() / np.abs(Y).max()
    print(f"{name}: |Q^T Q - I_kept|_max {orth:.2e} (LAPACK QR on the full-rank input {lapack_orth:.2e}), "
          f"|Q R - Y|_max / |Y|_max {res:.2e} (LAPACK {lapack_res:.2e})")
    assert orth <= max(100 * lapack_orth, n * EPS)
    assert res <= max(100 * lapack_res, n * EPS)


# ---- Jacobi ----------------------------------------------------------------------------------------------------------------
def _jacobi_input(name):
    rng = np.random.RandomState(len(name))
    if name == "zero_rows":
        A = rng.standard_normal((26, 26))
        A[[2, 9, 10, 25]] = 0.0
        return A
    c = int(name)
    return rng.standard_normal((c, c))


def _svd_defects(A, U, s, V, cols):
    """(residual, left defect, right defect) in the Frobenius norm; the right defect over the columns `cols`"""
    k = len(cols)
    return (np.linalg.norm((U * s) @ V.T - A), np.linalg.norm(U.T @ U - np.eye(U.shape[1])),
            np.linalg.norm(V[:, cols].T @ V[:, cols] - np.eye(k)))


@pytest.mark.parametrize("name", ["18", "160", "256", "zero_rows"])
def test_jacobi(name):
    from daisyrec_amd import _native as N, ops
    A = _jacobi_input(name)
    c = A.shape[0]
    Ul, sl, Vlt = np.linalg.svd(A)
    U, s, V, info = ops.psvd_jacobi(_dev(A))
    U, s, V, info = U.cpu().numpy(), s.cpu().numpy(), V.cpu().numpy(), info.cpu().numpy()
    assert info[0] == N.PSVD_CONVERGED and 1 <= info[1] <= 60
    assert (np.diff(s) <= 0).all() and (s >= 0).all()
    # a right vector of a zero singular value is returned as a zero column: zero_rows has exactly four
    cols = np.nonzero(s > 0)[0]
    assert len(cols) == (22 if name == "zero_rows" else c) and not V[:, len(cols):].any()
    floor = c * EPS * np.linalg.norm(A)
    got = _svd_defects(A, U, s, V, cols)
    lapack = _svd_defects(A, Ul, sl, Vlt.T, cols)
    s_err = np.abs(s - sl).max() / sl[0]
    print(f"jacobi {name}: {info[1]} sweeps, |s - s_lapack| / s_0 {s_err:.2e}, residual / left / right defect "
          f"{got[0]:.2e} {got[1]:.2e} {got[2]:.2e} (LAPACK {lapack[0]:.2e} {lapack[1]:.2e} {lapack[2]:.2e}), floor {floor:.2e}")
    assert s_err <= floor / sl[0]
    for mine, theirs in zip(got, lapack):
        assert mine <= max(16 * theirs, floor)


def test_jacobi_sweep_bound_is_reported():
    from daisyrec_amd import _native as N, ops
    info = ops.psvd_jacobi(_dev(_jacobi_input("160")), max_sweeps=1)[3].cpu().numpy()
    assert tuple(info) == (N.PSVD_NOT_CONVERGED, 1)


# ---- rank ------------------------------------------------------------------------------------------------------------------
def test_rank_orders_on_the_fp64_keys():
    from daisyrec_amd import ops
    I = 40
    perm = np.random.RandomState(0).permutation(I)
    item_vec = (1.0 + perm * 1e-12).reshape(I, 1)              # all equal in fp32, distinct in fp64
    assert len(np.unique(item_vec.astype(np.float32))) == 1 and len(np.unique(item_vec)) == I
    user_vec = np.array([[1.0], [-1.0]])
    cands = np.stack([np.arange(I), np.arange(I)[::-1]]).astype(np.int64)
    sc, ids = ops.psvd_rank(_dev(user_vec), _dev(item_vec), _dev([0, 1], torch.int64), _dev(cands, torch.int64), 10)
    want = user_vec @ item_vec.T
    assert np.array_equal(sc.cpu().numpy(), np.take_along_axis(want, cands, 1))
    assert np.array_equal(ids.cpu().numpy(), O.rank_lists(np.take_along_axis(want, cands, 1), cands, 10))


def test_rank_ties_clipping_and_full_rank():
    from daisyrec_amd import ops
    rng = np.random.RandomState(1)
    U, I, k = 5, 700, 3                                        # 700 items: more than one pass of the 256 threads
    user_vec, item_vec = rng.randint(-2, 3, (U, k)).astype(np.float64), rng.randint(-2, 3, (I, k)).astype(np.float64)
    full = user_vec @ item_vec.T                               # exact, with many exact ties
    uv, iv, users = _dev(user_vec), _dev(item_vec), _dev(np.arange(U), torch.int64)
    sc, ids = ops.psvd_rank(uv, iv, users, None, 50)
    assert np.array_equal(sc.cpu().numpy(), full)
    assert np.array_equal(ids.cpu().numpy(), np.argsort(-full, axis=1, kind="stable")[:, :50])
    cands = np.stack([rng.permutation(I)[:7] for _ in range(U)]).astype(np.int64)
    sc, ids = ops.psvd_rank(uv, iv, users, _dev(cands, torch.int64), 10)          # topk >= cand_num: clipped
    assert ids.shape == (U, 7)
    assert np.array_equal(ids.cpu().numpy(), O.rank_lists(np.take_along_axis(full, cands, 1), cands, 7))
    sc, ids = ops.psvd_rank(uv, iv, users, _dev(cands, torch.int64), 0)           # scores only
    assert ids is None and np.array_equal(sc.cpu().numpy(), np.take_along_axis(full, cands, 1))


# ---- the model end to end -----------------------------------------------------------------------------------------------------
def _frame(c):
    import pandas as pd
    return pd.DataFrame({"user": c["u"], "item": c["i"], "rating": c["r"]})


def _fit(tag):
    from daisyrec_amd.model import PureSVD
    c = case(tag)
    m = PureSVD(puresvd_config(user_num=c["U"], item_num=c["I"], factors=c["factors"], topk=TOPK))
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
    c, m, f = case(tag), fitted(tag), oracle_fit(tag, "cholqr2")
    sc = m._rank(np.arange(c["U"]), np.array(c["cands"]))[0].cpu().numpy()
    dev = np.abs(sc - c["scores_ref"]).max()
    print(f"{tag}: max |score - reference| {dev:.2e} = {dev / (c['tol'] / 100):.2f} x oracle_dev (allowed: 100), Jacobi sweeps "
          f"{m.fit_info['jacobi_sweeps']}")
    assert dev <= c["tol"]
    assert np.abs(m.fit_info["sigma"] - c["sigma"]).max() <= c["tol"] / c["score_max"] * c["sigma"][0]
    assert m.fit_info["n_iter"] == f["n_iter"] and m.fit_info["transposed"] == f["transposed"]
    assert m.fit_info["dropped"] == f["dropped"]
    user_vec, item_vec = m.user_vec, m.item_vec
    assert user_vec.dtype == item_vec.dtype == np.float64
    assert user_vec.shape == (c["U"], c["factors"]) and item_vec.shape == (c["I"], c["factors"])
    ok = O.separated(c["sigma"])
    print(f"{tag}: {int((~ok).sum())} components skipped in the vector comparison")
    assert ok.all() or not c["ranked"]
    for mine, gold in ((user_vec, c["user_vec"]), (item_vec, c["item_vec"])):
        vdev = np.abs(mine[:gold.shape[0]] - gold)[:, ok].max()
        print(f"{tag}: max |vector - reference| {vdev:.2e} = {vdev / (c['vec_tol'] / 100):.2f} x oracle_vec_dev")
        assert vdev <= c["vec_tol"]
    top = user_vec[np.argmax(np.abs(user_vec), axis=0), np.arange(c["factors"])]
    assert (top[ok] > 0).all()                                  # svd_flip's sign rule
    if c["ranked"]:
        ranks = m.rank(_loader(c))
        assert ranks.dtype == np.int64 and np.array_equal(ranks, c["rank_ref"])


@pytest.mark.parametrize("tag", ["tiny", "wide"])
def test_predict_and_full_rank_agree_with_the_scores(tag):
    c, m = case(tag), fitted(tag)
    full = m._rank(np.arange(c["U"]))[0].cpu().numpy()
    assert np.abs(full - m.user_vec @ m.item_vec.T).max() <= c["tol"]
    for u in (0, c["U"] - 1):
        got = m.full_rank(u)
        assert got.dtype == np.int64 and np.array_equal(got, np.argsort(-full[u], kind="stable")[:TOPK])
        for i in (0, int(c["cands"][u, 0])):
            p = m.predict(u, i)
            assert isinstance(p, float) and p == full[u, i]
    with pytest.raises(IndexError):
        m.predict(c["U"], 0)


@pytest.mark.parametrize("tag", ["fewitems", "default_r"])
def test_second_fit_is_bitwise_identical(tag):
    a, b = fitted(tag), _fit(tag)
    assert torch.equal(a._user_vec, b._user_vec) and torch.equal(a._item_vec, b._item_vec)
    assert a.fit_info["dropped"] == b.fit_info["dropped"] and a.fit_info["jacobi_sweeps"] == b.fit_info["jacobi_sweeps"]


def test_calls_before_fit_are_refused():
    from daisyrec_amd.model import PureSVD
    m = PureSVD(puresvd_config())
    with pytest.raises(RuntimeError, match="fit"):
        m.full_rank(0)


def test_user_without_training_rows_scores_exactly_zero():
    """An empty row of X stays zero through every product: the user's vector is exactly zero, all of its scores tie and
    its list is the first topk candidates (the reference leaves rounding noise there and ranks by it: DESIGN.md §16)."""
    from daisyrec_amd.model import PureSVD
    c = case("tiny")
    keep = (c["u"] != 5) & (c["i"] != 7)                      # user 5 and item 7 lose every interaction
    import pandas as pd
    m = PureSVD(puresvd_config(user_num=c["U"], item_num=c["I"], factors=c["factors"], topk=TOPK))
    m.fit(pd.DataFrame({"user": c["u"][keep], "item": c["i"][keep], "rating": c["r"][keep]}))
    assert not m.user_vec[5].any() and not m.item_vec[7].any()
    assert np.isfinite(m.user_vec).all() and np.isfinite(m.item_vec).all() and m.fit_info["dropped"] == [0] * 10
    cands = np.array(c["cands"][5:6])
    ranks = m.rank([(torch.tensor([5]), torch.from_numpy(cands))])
    assert np.array_equal(ranks, cands[:, :TOPK])
