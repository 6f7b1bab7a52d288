"""ops.walk2_topk (csrc/walk2.hip) and the RP3beta / P3alpha models against tests/rp3_oracle.py.  The
kernel's order of operations is fixed and the oracle repeats it, so every kernel test compares by EQUALITY: counts, columns
and the bits of the values."""
import functools
import logging

import numpy as np
import pytest
import torch

import rp3_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
U, I, K = O.U, O.I, 10


def _dev_csr(csr):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in csr)


def run(A, B, n_cols, k, scale=None, **kw):
    from daisyrec_amd import ops
    s = None if scale is None else torch.from_numpy(np.asarray(scale, dtype=np.float32)).to(DEV)
    return tuple(t.cpu().numpy() for t in ops.walk2_topk(_dev_csr(A), _dev_csr(B), n_cols, k, s, **kw))


def same(got, want):
    """counts, columns and the BITS of the values"""
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float32
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[2].view(np.uint32), np.ascontiguousarray(want[2]).view(np.uint32))


# ---- the cases, each with its oracle result computed once ------------------------------------------------------------
@functools.lru_cache(None)
def dyadic():
    X, A, B, scale = O.dyadic_case()
    return A, B, scale, O.walk2_topk(A, B, I, K, scale)


@functools.lru_cache(None)
def real_case():
    """real-valued operands and scales: the model's own arithmetic at alpha = 0.7, beta = 0.4 on ratings 1..5"""
    X = O.pattern(3).astype(np.float64) * np.random.default_rng(4).integers(1, 6, (U, I))
    Piu, Pui = O.model_operands(X, 0.7)
    return Piu, Pui, O.model_scales(X, 0.7, 0.4)[2]


@functools.lru_cache(None)
def real_want(k, zero_diagonal=True, normalize=False, scaled=True):
    A, B, scale = real_case()
    return O.walk2_topk(A, B, I, k, scale if scaled else None, zero_diagonal=zero_diagonal, normalize=normalize)


@functools.lru_cache(None)
def long_rows_case():
    """3000 x 1500 with a user of 700 items (a row of B longer than the 256 lanes of a workgroup) and an item with all
    3000 users (a source row longer than the 64 entries a wave takes at a time)"""
    rng = np.random.default_rng(11)
    X = rng.random((3000, 1500)) < 0.002
    X[7, rng.choice(1500, 700, replace=False)] = True
    X[:, 11] = True
    val = rng.random((3000, 1500)) + 0.5
    A = O.csr_pattern(X.T, values=val.T)
    B = O.csr_pattern(X, values=val)
    scale = (rng.random(1500) + 0.25).astype(np.float32)
    return A, B, scale


@functools.lru_cache(None)
def long_rows_want(k):
    A, B, scale = long_rows_case()
    return O.walk2_topk(A, B, 1500, k, scale)


@functools.lru_cache(None)
def wide_case(n_cols):
    """64 source rows over 500 inner ids and n_cols columns, a few thousand entries, signed values"""
    rng = np.random.default_rng(n_cols)
    A = O.csr_of((rng.random((64, 500)) < 0.05) * rng.standard_normal((64, 500)))
    col = np.concatenate([np.append(np.sort(rng.choice(n_cols - 1, 8, replace=False)), n_cols - 1) for _ in range(500)])
    val = rng.standard_normal((500, 9))
    val[:, 8] = 1.0                                          # the last column is reached from every inner id
    B = np.arange(501, dtype=np.int64) * 9, col.astype(np.int32), val.reshape(-1).astype(np.float32)
    return A, B, O.walk2_topk(A, B, n_cols, 16, None, zero_diagonal=False)


# ---- the kernel ------------------------------------------------------------------------------------------------------
def test_dyadic_case_against_the_oracle_and_exact_arithmetic():
    A, B, scale, want = dyadic()
    got = run(A, B, I, K, scale)
    same(got, want)
    full = (O.dense_of(A, U) @ O.dense_of(B, I)) * scale.astype(np.float64)[None, :]          # fp64, every sum exact
    np.fill_diagonal(full, 0.0)
    ints = full * 2.0 ** 20                                  # ... and an integer once scaled by a power of two
    assert np.array_equal(ints, np.round(ints))
    for i in range(I):
        c = got[0][i]
        order = np.lexsort((np.arange(I), -full[i]))[:K]
        keep = np.sort(order[full[i, order] > 0])
        assert np.array_equal(got[1][i, :c], keep) and np.array_equal(got[2][i, :c].astype(np.float64), full[i, keep])


@pytest.mark.parametrize("path", ["lds", "global"])
def test_real_values_under_both_paths(path):
    A, B, scale = real_case()
    same(run(A, B, I, K, scale, path=path), real_want(K))


@pytest.mark.parametrize("k", [1, I, I + 56])
def test_k_of_one_and_k_beyond_the_columns(k):
    A, B, scale = real_case()
    got = run(A, B, I, k, scale)
    same(got, real_want(k))
    assert got[1].shape == (I, k)
    if k >= I:
        assert got[0].max() < I                              # the diagonal is never kept


def test_largest_k_and_rows_longer_than_a_workgroup_or_a_chunk():
    from daisyrec_amd import _native as N
    A, B, scale = long_rows_case()
    assert np.diff(B[0]).max() >= 700 and np.diff(A[0]).max() == 3000
    got = run(A, B, 1500, N.KNN_MAX_K, scale)
    same(got, long_rows_want(N.KNN_MAX_K))
    assert got[0].max() == N.KNN_MAX_K and got[0][11] == N.KNN_MAX_K
    same(run(A, B, 1500, N.KNN_MAX_K, scale, path="global"), long_rows_want(N.KNN_MAX_K))
    same(run(A, B, 1500, 50, scale), long_rows_want(50))


def test_degenerate_rows():
    """item 5: nobody used it; item 4: its only user has no other item (only the diagonal is reached); item 0: two
    positive weights, fewer than K = 3; user 4 has no item at all"""
    X = np.zeros((5, 8), dtype=bool)
    X[0, [0, 1, 2]] = X[1, [1, 2, 3]] = X[3, [1, 6, 7]] = True
    X[2, 4] = True
    A, B = O.csr_pattern(X.T), O.csr_pattern(X)
    want = O.walk2_topk(A, B, 8, 3)
    for path in ("lds", "global"):
        got = run(A, B, 8, 3, path=path)
        same(got, want)
        assert got[0].tolist() == [2, 3, 3, 2, 0, 0, 2, 2]
        assert got[1][0].tolist() == [1, 2, -1] and got[2][0].tolist() == [1.0, 1.0, 0.0]
        assert np.all(got[1][4] == -1) and np.all(got[2][5] == 0)


@pytest.mark.parametrize("zero_diagonal", [True, False])
@pytest.mark.parametrize("n_rows", [150, 250])
def test_rectangular_operands(n_rows, zero_diagonal):
    """n_rows != n_cols on either side, signed values: negative sums are never kept"""
    rng = np.random.default_rng(n_rows)
    A = O.csr_of((rng.random((n_rows, 300)) < 0.06) * rng.standard_normal((n_rows, 300)))
    B = O.csr_of((rng.random((300, 200)) < 0.08) * rng.standard_normal((300, 200)))
    scale = (rng.random(200) + 0.5).astype(np.float32)
    want = O.walk2_topk(A, B, 200, 12, scale, zero_diagonal=zero_diagonal)
    got = run(A, B, 200, 12, scale, zero_diagonal=zero_diagonal)
    same(got, want)
    assert np.all(got[2][got[1] >= 0] > 0)
    rows = np.arange(min(n_rows, 200))
    assert zero_diagonal != bool((got[1][rows] == rows[:, None]).any())


def test_normalize_and_no_column_scale():
    A, B, scale = real_case()
    got = run(A, B, I, K, scale, normalize=True)
    same(got, real_want(K, normalize=True))
    assert np.allclose(got[2].sum(1)[got[0] > 0], 1.0, atol=1e-6)
    same(run(A, B, I, K, None), real_want(K, scaled=False))
    same(run(A, B, I, K, None, normalize=True, zero_diagonal=False, path="global"),
         O.walk2_topk(A, B, I, K, None, zero_diagonal=False, normalize=True))


def test_beyond_the_lds_limit_auto_takes_the_global_path():
    from daisyrec_amd import _native as N
    n_cols = N.WALK2_LDS_COLS + 17
    A, B, want = wide_case(n_cols)
    auto, lds_ws = N.SLIM_PATHS["auto"], N.lib.daisy_walk2_workspace_bytes(64, N.WALK2_LDS_COLS, N.SLIM_PATHS["auto"], 0)
    assert N.lib.daisy_walk2_workspace_bytes(64, n_cols, auto, 0) >= lds_ws + 64 * n_cols * 4          # the slabs
    assert N.lib.daisy_walk2_workspace_bytes(64, n_cols, auto, 0) == N.lib.daisy_walk2_workspace_bytes(
        64, n_cols, N.SLIM_PATHS["global"], 0)
    got = run(A, B, n_cols, 16, zero_diagonal=False)
    same(got, want)
    assert (got[1] == n_cols - 1).any()                      # a column past the LDS limit is kept
    with pytest.raises(ValueError, match="LDS path holds at most"):
        run(A, B, n_cols, 16, path="lds")


def test_the_whole_lds_budget():
    from daisyrec_amd import _native as N
    n_cols = N.WALK2_LDS_COLS
    A, B, want = wide_case(n_cols)
    assert N.lib.daisy_walk2_workspace_bytes(64, n_cols, N.SLIM_PATHS["auto"], 0) == \
        N.lib.daisy_walk2_workspace_bytes(64, n_cols, N.SLIM_PATHS["lds"], 0)
    same(run(A, B, n_cols, 16, zero_diagonal=False), want)
    same(run(A, B, n_cols, 16, zero_diagonal=False, path="global"), want)


def test_global_path_two_runs_and_group_counts_are_bit_equal():
    A, B, scale, want = dyadic()
    for kw in ({"path": "global"}, {"path": "lds"}, {"groups": 1}, {"groups": 3}, {"groups": 1, "path": "global"},
               {"groups": 7, "path": "global"}, {"groups": 4096}):
        same(run(A, B, I, K, scale, **kw), want)
    A, B, scale = long_rows_case()
    first = run(A, B, 1500, 50, scale)
    same(run(A, B, 1500, 50, scale), first)
    same(run(A, B, 1500, 50, scale, groups=5, path="global"), first)


def test_argument_errors():
    from daisyrec_amd import ops
    A, B, scale, _ = dyadic()
    for k in (0, -3, ops.N.KNN_MAX_K + 1):
        with pytest.raises(ValueError, match="K="):
            run(A, B, I, k, scale)
    with pytest.raises(ValueError, match="path"):
        run(A, B, I, K, scale, path="shared")
    with pytest.raises(ValueError, match="n_groups"):
        run(A, B, I, K, scale, groups=-1)
    with pytest.raises(ValueError, match="col_scale"):
        run(A, B, I, K, scale[:-1])
    ptr, col, val = B
    lo = int(ptr[3])
    assert ptr[4] - lo >= 2
    swapped, twice, far = col.copy(), col.copy(), col.copy()
    swapped[[lo, lo + 1]] = swapped[[lo + 1, lo]]
    twice[lo + 1] = twice[lo]
    far[lo] = I
    for bad, what in ((swapped, "ascending"), (twice, "ascending"), (far, "outside")):
        with pytest.raises(ValueError, match=what):
            run(A, (ptr, bad, val), I, K, scale)
    a_far = A[1].copy()
    a_far[0] = U
    with pytest.raises(IndexError):
        run((A[0], a_far, A[2]), B, I, K, scale)
    need = ops.lib.daisy_walk2_workspace_bytes(I, I, ops.N.SLIM_PATHS["global"], 0)
    small = torch.empty(need - 1, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="workspace"):
        run(A, B, I, K, scale, path="global", workspace=small)
    same(run(A, B, I, K, scale, path="global", workspace=torch.empty(need, dtype=torch.uint8, device=DEV)), dyadic()[3])


# ---- the models on the ml-100k training pairs ------------------------------------------------------------------------
TOPK, MAXK = 10, 100


def rp3_config(**over):
    cfg = {"gpu": "0", "logger": logging.getLogger("rp3-test"), "user_num": 943, "item_num": 1152, "topk": TOPK, "maxk": MAXK}
    cfg.update(over)
    return cfg


@functools.lru_cache(None)
def pairs():
    import os
    from conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, "ml100k_c1.npz"))
    return g["train_users"].astype(np.int64), g["train_items"].astype(np.int64)


def frame(ratings=None):
    import pandas as pd
    users, items = pairs()
    return pd.DataFrame({"user": users, "item": items, "rating": np.ones(len(users)) if ratings is None else ratings})


@functools.lru_cache(None)
def int_ratings():
    return np.random.default_rng(21).integers(1, 6, len(pairs()[0])).astype(np.float64)


@functools.lru_cache(None)
def fitted(cls="RP3beta", explicit=False, **over):
    from daisyrec_amd import model as M
    m = getattr(M, cls)(rp3_config(**over, **({"implicit": False} if explicit else {})))
    m.fit(frame(int_ratings() if explicit else None))
    return m


def dense_X(ratings=None):
    users, items = pairs()
    X = np.zeros((943, 1152))
    np.add.at(X, (users, items), 1.0 if ratings is None else ratings)
    return X


def _np_csr(csr):
    return tuple(t.cpu().numpy() for t in csr)


def _ulp_close(got, want):
    """within one float32 ulp of the float64 value rounded to float32"""
    want = np.asarray(want, dtype=np.float32)
    return np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(want).astype(np.float64))


@functools.lru_cache(None)
def oracle_W(cls="RP3beta", explicit=False, **over):
    """the oracle walk on the model's own operands and scales -> W dense float64 [I, I]"""
    m = fitted(cls, explicit, **over)
    Piu, Pui = (_np_csr(c) for c in m._P)
    res = O.walk2_topk(Piu, Pui, 1152, min(m.k, 1152), m.scales[2].cpu().numpy(), normalize=m.normalize_similarity)
    return O.dense_rows(*res, 1152)


@functools.lru_cache(None)
def oracle_scores():
    return O.scores(dense_X(), oracle_W())


def test_scales_within_one_ulp_of_numpy():
    m = fitted()
    X = dense_X()
    want = O.model_scales(X, m.alpha, m.beta)
    assert (m.alpha, m.beta, m.k, m.implicit, m.normalize_similarity) == (1.0, 0.6, MAXK, True, False)
    for got, w in zip(m.scales, want):
        assert got.dtype == torch.float32 and _ulp_close(got.cpu().numpy(), w)
    m7 = fitted(alpha=0.7, beta=0.4)
    for got, w in zip(m7.scales, O.model_scales(X, 0.7, 0.4)):
        assert _ulp_close(got.cpu().numpy(), w)
    # implicit: an operand's entry IS its row's scale
    Piu, Pui = (_np_csr(c) for c in m7._P)
    assert np.array_equal(Pui[2], np.repeat(m7.scales[0].cpu().numpy(), np.diff(Pui[0])))
    assert np.array_equal(Piu[2], np.repeat(m7.scales[1].cpu().numpy(), np.diff(Piu[0])))
    deg_u = np.diff(Pui[0])
    assert m.fit_info["paths"] == int((deg_u.astype(np.int64) ** 2).sum()) and m.fit_info["n"] == 1152


@pytest.mark.parametrize("over", [(), (("alpha", 0.7), ("beta", 0.4))])
def test_w_sparse_equals_the_oracle_fed_with_the_models_scales(over):
    import scipy.sparse as sp
    m = fitted(**dict(over))
    W = m.w_sparse
    assert sp.isspmatrix_csc(W) and W.dtype == np.float32 and W.shape == (1152, 1152)
    want = oracle_W(**dict(over))
    assert np.array_equal(np.asarray(W.todense()).astype(np.float64), want)
    assert m.fit_info["nnz"] == W.nnz == int((want != 0).sum()) and m.fit_info["bytes_held"] >= W.nnz * 8
    assert (W.getnnz(axis=1) <= MAXK).all() and W.diagonal().sum() == 0


def test_scores_and_lists_equal_the_oracles_fp64_scores_and_order():
    from daisyrec_amd.utils.utils import _ur_pairs, user_csr
    m, S = fitted(), oracle_scores()
    every = np.arange(943)
    full, ids = m._rank(every, None, TOPK)
    assert np.array_equal(full.cpu().numpy(), S)
    want_ids = np.stack([O.top_ids(S[u], TOPK) for u in every])
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    for u, i in ((0, 0), (5, 100), (942, 1151)):
        p = m.predict(u, i)
        assert isinstance(p, float) and p == S[u, i]
        assert np.array_equal(m.full_rank(u), want_ids[u])
    rng = np.random.default_rng(2)
    us, cands = np.arange(0, 943, 37), rng.integers(0, 1152, (26, 40))
    got = m.rank([(torch.from_numpy(us[:13]), torch.from_numpy(cands[:13])), (torch.from_numpy(us[13:]), torch.from_numpy(cands[13:]))])
    assert got.dtype == np.int64
    assert np.array_equal(got, np.stack([O.top_ids(S[u, c], TOPK, c) for u, c in zip(us, cands)]))
    # full_rank_users / full_rank_positions without the training items
    users, items = pairs()
    train_ur = {u: set(items[users == u].tolist()) for u in range(943)}
    test_ur = {u: {int(t) for t in rng.choice(sorted(set(range(1152)) - train_ur[u]), 2, replace=False)} for u in range(0, 943, 9)}
    some = np.array(sorted(test_ur))
    lists, sc = m.full_rank_users(torch.from_numpy(some).to(DEV), exclude=train_ur, return_scores=True)
    lists, sc = lists.cpu().numpy(), sc.cpu().numpy()
    out = m.full_rank_positions(torch.from_numpy(some).to(DEV), test_ur, exclude=train_ur, return_scores=True, return_eligible=True)
    indptr, pos, tsc, elig = (t.cpu().numpy() for t in out)
    for b, u in enumerate(some):
        masked = S[u].copy()
        masked[sorted(train_ur[u])] = -np.inf
        want = O.top_ids(masked, TOPK)
        assert np.array_equal(lists[b], want) and np.array_equal(sc[b], S[u, want])
        assert elig[b] == 1152 - len(train_ur[u])
        order = np.lexsort((np.arange(1152), -masked))
        for slot, t in zip(range(indptr[b], indptr[b + 1]), sorted(test_ur[u])):
            assert pos[slot] == int(np.flatnonzero(order == t)[0]) and tsc[slot] == S[u, t]


def test_p3alpha_is_rp3beta_without_the_penalty():
    a, b = fitted("P3alpha", alpha=0.8), fitted(alpha=0.8, beta=0.0)
    assert a.beta == 0.0 and torch.equal(a.scales[2], (a.scales[2] > 0).to(torch.float32))
    assert all(torch.equal(x, y) for x, y in zip(a._W, b._W))
    assert torch.equal(a._rank(np.arange(50), None, 0)[0], b._rank(np.arange(50), None, 0)[0])
    assert not all(torch.equal(x, y) for x, y in zip(a._W, fitted(alpha=0.8, beta=0.4)._W))
    assert fitted("P3alpha", alpha=0.8, beta=0.9).beta == 0.0            # P3alpha has no beta to set


def test_explicit_integer_ratings():
    m = fitted(explicit=True, alpha=0.7, beta=0.4)
    X = dense_X(int_ratings())
    for got, w in zip(m.scales, O.model_scales(X, 0.7, 0.4)):
        assert _ulp_close(got.cpu().numpy(), w)
    for got, w in zip(m._P, O.model_operands(X, 0.7)):
        got = _np_csr(got)
        assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1]) and _ulp_close(got[2], w[2].astype(np.float64))
    W = oracle_W(explicit=True, alpha=0.7, beta=0.4)
    assert np.array_equal(np.asarray(m.w_sparse.todense()).astype(np.float64), W)
    users = np.arange(0, 943, 50)
    assert np.array_equal(m._rank(users, None, 0)[0].cpu().numpy(), O.scores(X[users], W))
    from daisyrec_amd.model import RP3beta
    with pytest.raises(ValueError, match="ratings > 0"):
        RP3beta(rp3_config(implicit=False)).fit(frame(int_ratings() - 1))


def test_normalize_similarity():
    m = fitted(normalize_similarity=True)
    W = np.asarray(m.w_sparse.todense()).astype(np.float64)
    assert np.array_equal(W, oracle_W(normalize_similarity=True))
    sums = W.sum(1)
    assert np.allclose(sums[sums > 0], 1.0, atol=1e-5) and np.array_equal((W != 0), (oracle_W() != 0))


def test_second_fit_is_bitwise_identical():
    from daisyrec_amd.model import RP3beta
    a = fitted()
    b = RP3beta(rp3_config())
    b.fit(frame())
    assert all(torch.equal(x, y) for x, y in zip(a._W, b._W))


def test_calc_full_ranking_results_returns_a_frame(tmp_path):
    from daisyrec_amd.utils.metrics import calc_full_ranking_results
    m = fitted()
    users, items = pairs()
    rng = np.random.default_rng(8)
    train_ur = {u: set(items[users == u].tolist()) for u in range(943)}
    test_ur = {u: {int(rng.choice(sorted(set(range(1152)) - train_ur[u])))} for u in range(0, 943, 5)}
    cfg = {"logger": logging.getLogger("rp3-test"), "res_path": str(tmp_path / "res"), "item_num": 1152, "topk": TOPK,
           "metrics": ["recall", "ndcg", "full_auc"]}
    res = calc_full_ranking_results(m, test_ur, train_ur, cfg)
    assert list(res.columns) == ["KPI@K", 1, 5, 10] and len(res) == 3 and np.isfinite(res[10].to_numpy()).all()


def test_the_unfitted_model_and_bad_config_values_raise():
    from daisyrec_amd.model import P3alpha, RP3beta
    for cls in (RP3beta, P3alpha):
        m = cls(rp3_config())
        assert m.w_sparse is None and m.pred_mat is None and m.fit_info is None and m.scales is None
        for call in (lambda: m.full_rank(0), lambda: m.predict(0, 0), lambda: m.rank([]),
                     lambda: m.full_rank_users(torch.arange(2, device=DEV))):
            with pytest.raises(RuntimeError, match="fit"):
                call()
    for bad in ({"alpha": -0.1}, {"beta": -1.0}, {"alpha": float("nan")}, {"beta": float("inf")}, {"maxk": 0}, {"topk": 0},
                {"user_num": 0}, {"item_num": 0}):
        with pytest.raises(ValueError):
            RP3beta(rp3_config(**bad))
    with pytest.raises(KeyError):
        RP3beta({"gpu": "0", "user_num": 3, "item_num": 3})
    with pytest.raises(ValueError, match="above"):
        RP3beta(rp3_config(maxk=5000, item_num=2000)).fit(frame())
    with pytest.raises(ValueError, match="outside"):
        RP3beta(rp3_config(item_num=1000)).fit(frame())
