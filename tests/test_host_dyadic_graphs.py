"""tests/dyadic_graphs.py without a GPU: on the default biregular graph the oracle's normalised adjacency holds powers of
two only, the products tests/test_gpu_graph_products_exact.py asks for are fp32 numbers in any summation order, and
`assert_exact_domain` refuses the graphs and inputs for which that does not hold."""
import numpy as np
import pytest
import scipy.sparse as sp

import dyadic_graphs as DG
from oracle import lightgcn_numpy as LG
from oracle import neumf_numpy as NM

NODE_STREAM = 0x100          # DAISY_NGCF_NODE_STREAM (daisyrec_amd._native.NGCF_NODE_STREAM)
SEED = 0x5EED0001


@pytest.fixture(scope="module")
def default():
    gu, gi, U, I, spans = DG.biregular()
    indptr, col, val = LG.norm_adj_csr(gu, gi, U, I)
    row = np.repeat(np.arange(U + I), np.diff(indptr))
    return dict(gu=gu, gi=gi, U=U, I=I, N=U + I, spans=spans, indptr=indptr, row=row, col=col, val=val)


def _fits_fp32(x):
    return np.array_equal(x.astype(np.float32).astype(np.float64), x)


def test_default_graph_is_dyadic(default):
    g = default
    assert (g["U"], g["I"], len(g["val"])) == (2051, 2003, 61248)
    assert len(np.unique(g["gu"].astype(np.int64) * g["I"] + g["gi"])) == len(g["gu"]) == 30624       # distinct pairs
    assert g["val"].dtype == np.float32
    assert set(np.unique(g["val"]).tolist()) == {2.0 ** -k for k in range(2, 7)}
    deg = np.diff(g["indptr"])
    assert tuple(np.unique(deg).tolist()) == DG.DEFAULT_DEGREES
    for block in (deg[:g["U"]], deg[g["U"]:]):
        assert block[0] == 0 and block[-1] == 0                                  # isolated first and last rows
        assert {256, 512, 1024} <= set(block.tolist())                           # 1, 2 and 4 segments on either side
    for (a, b, nu), (u0, n_u, i0, n_i) in zip(DG.DEFAULT_COMPONENTS, g["spans"]):
        assert (deg[u0:u0 + n_u] == a).all() and (deg[g["U"] + i0:g["U"] + i0 + n_i] == b).all()
        assert deg[u0 - 1] == 0 and deg[g["U"] + i0 - 1] == 0                    # the gap before every component
        k = np.log2(a * b) / 2
        assert k == int(k) and (g["val"][g["indptr"][u0]:g["indptr"][u0 + n_u]] == 2.0 ** -k).all()


def test_gap_and_bad_components():
    gu, gi, U, I, spans = DG.biregular(((4, 4, 8), (8, 8, 8)), gap=3)
    assert (U, I) == (8 + 8 + 9, 8 + 8 + 9) and spans[0][0] == 3 and spans[1][0] == 14
    with pytest.raises(ValueError):
        DG.biregular(((4, 16, 2),))              # 8 links do not divide into items of degree 16
    with pytest.raises(ValueError):
        DG.biregular(((8, 8, 4),))               # a user of degree 8 over 4 items


def test_products_are_fp32_numbers_in_any_order(default):
    g, N, d = default, default["N"], 512
    rng = np.random.default_rng(1)
    X = rng.integers(-8, 9, (N, d)).astype(np.float64)
    nnz = len(g["val"])
    for p in (0.0, 0.5, 0.75):
        scale = 1.0 / (1.0 - p)
        DG.assert_exact_domain((g["row"], g["col"], g["val"]), X, scale)
        keep = NM.drop_keep(SEED, NODE_STREAM, np.arange(nnz), p) if p else np.ones(nnz, bool)
        assert p == 0 or abs(keep.mean() - (1 - p)) < 0.02
        w = np.where(keep, g["val"].astype(np.float64) * scale, 0.0)
        A = sp.csr_matrix((w, (g["row"], g["col"])), shape=(N, N))
        for M in (A, A.T.tocsr()):
            Y = M @ X
            assert _fits_fp32(Y)
            if p == 0.75 or M is A:
                # the same sum in fp32, entry by entry in a shuffled order
                coo = M.tocoo()
                order = rng.permutation(coo.nnz)
                r, c, v = coo.row[order], coo.col[order], coo.data[order].astype(np.float32)
                cols = slice(0, 64)
                out = np.zeros((N, 64), np.float32)
                np.add.at(out, r, v[:, None] * X[c, cols].astype(np.float32))
                assert np.array_equal(out.view(np.uint32), (Y[:, cols] + 0.0).astype(np.float32).view(np.uint32))


def test_irregular_graph_and_its_twin():
    gu, gi, U, I = DG.irregular()
    assert U == len(DG.IRREGULAR_LENGTHS) and I == 1037
    assert len(np.unique(gu.astype(np.int64) * I + gi)) == len(gu) == sum(DG.IRREGULAR_LENGTHS)
    assert np.array_equal(np.bincount(gu, minlength=U), DG.IRREGULAR_LENGTHS)
    indptr, _, _ = LG.norm_adj_csr(gi, gu, I, U)                   # the twin: the long rows come last
    assert np.array_equal(np.diff(indptr)[I:], DG.IRREGULAR_LENGTHS)
    assert indptr[I] == len(gu)


def test_the_guard_rejects_what_is_not_exact(default):
    g = default
    coo = (g["row"], g["col"], g["val"])
    X = np.ones((g["N"], 4))
    DG.assert_exact_domain(coo, X, 4.0, prefill=8 * X)
    with pytest.raises(AssertionError, match="2\\^24"):
        DG.assert_exact_domain(coo, X * 4096, 4.0)                 # 4096 * 1024 * 4 = 2^24
    DG.assert_exact_domain(coo, X * 4095, 4.0)
    with pytest.raises(AssertionError, match="2\\^24"):
        DG.assert_exact_domain(coo, X, 1.0, prefill=X * (1 << 18))     # 2^18 / 2^-6
    with pytest.raises(AssertionError, match="2\\^24"):
        DG.assert_exact_domain(coo, X * 2048, 4.0, halved=True)
    with pytest.raises(AssertionError, match="integers"):
        DG.assert_exact_domain(coo, X * 0.5, 1.0)
    with pytest.raises(AssertionError, match="scale"):
        DG.assert_exact_domain(coo, X, 1.0 / 0.7)
    # a (2, 8) component: 2 * 8 = 4^2, but 0.5e-7 * (1 / 2 + 1 / 8) is more than the half-ulp 2^-25
    gu, gi, U, I, _ = DG.biregular(((2, 8, 8),))
    indptr, col, val = LG.norm_adj_csr(gu, gi, U, I)
    row = np.repeat(np.arange(U + I), np.diff(indptr))
    assert (val < 0.25).all() and (val > 0.2499).all()
    with pytest.raises(AssertionError, match="powers of two"):
        DG.assert_exact_domain((row, col, val), np.ones((U + I, 4)), 1.0)
    # two components merged into one graph with mixed degrees: rows with more than one coefficient
    gu, gi, U, I = DG.irregular((4, 4, 16, 16))
    indptr, col, val = LG.norm_adj_csr(gu, gi, U, I)
    row = np.repeat(np.arange(U + I), np.diff(indptr))
    with pytest.raises(AssertionError):
        DG.assert_exact_domain((row, col, val), np.ones((U + I, 4)), 1.0)
