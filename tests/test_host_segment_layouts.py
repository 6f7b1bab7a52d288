"""tests/segment_layouts.py without a GPU: the layouts are what they say, `batch` reproduces them, `exact_step` is the
project's oracle (oracle.bpr_mf_numpy.mf_sgd_step) bit for bit, and every case tests/test_gpu_segment_layouts.py runs lies
inside the domain in which fp32 sums do not depend on their order."""
import numpy as np
import pytest

import segment_layouts as S
from oracle import bpr_mf_numpy as O


@pytest.mark.parametrize("n", [1, 2, 3, 129, 256, 512, 2049, 4096, 8192, 65536])
def test_layouts_are_positive_and_sum_to_n(n):
    names = set()
    for name, lens in S.layouts(n):
        assert name not in names
        names.add(name)
        assert min(lens) >= 1 and sum(lens) == n, (n, name)
    assert "one" in names and (n == 1 or "ones" in names)
    if n >= 2 * S.PERIODS[-1]:                  # nothing collapses: every layout of the family is there
        for p in S.PERIODS[1:]:
            assert {f"period({p},0)", f"period({p},1)", f"comb(1,{p})"} <= names, p
            assert p == 2 or {f"period({p},{p - 1})", f"comb(1,{p - 1})"} <= names, p
        assert {"long(0)", "long(1)", "long(3)"} & names == {"long(1)", "long(3)"}      # long(0) is `one`


def test_layout_shapes():
    assert S.period(10, 4, 0) == [4, 4, 2] and S.period(10, 4, 1) == [1, 4, 4, 1] and S.period(10, 4, 3) == [3, 4, 3]
    assert S.period(8, 4, 0) == [4, 4] and S.period(2, 4, 0) == [2] and S.period(4, 4, 4) is None
    assert S.comb(10, 1, 3) == [1, 3, 1, 3, 1, 1] and S.comb(9, 1, 4) == [1, 4, 1, 3]
    assert S.long(10, 3) == [1, 1, 1, 4, 1, 1, 1] and S.long(10, 0) == [10] and S.long(6, 3) is None
    assert [name for name, _ in S.layouts(2)] == ["one", "ones"]
    # n = p + 1: a last chunk of one entry
    assert S.named(129, "period(128,0)") == [128, 1] and S.named(257, "period(256,1)") == [1, 256]
    assert S.LARGEST_CHUNK <= S.PERIODS[-1]
    ids = S.row_ids(7)
    assert list(ids) == [0, 1, 3, 4, 6, 7, 9] and S.rows_needed(7) > ids[-1] + 1 and not (ids % 3 == 2).any()


@pytest.mark.parametrize("pointwise", [False, True])
@pytest.mark.parametrize("B", [1, 2, 129, 4096])
def test_batch_reproduces_the_layouts(B, pointwise):
    E = B if pointwise else 2 * B
    rng = np.random.default_rng(B)
    for name, lu, li in S._pair(list(S.layouts(B)), list(S.layouts(E))):
        u, i, j, U, I = S.batch(lu, li, rng, pointwise)
        assert u.dtype == i.dtype == j.dtype == np.int32 and len(u) == len(i) == len(j) == B
        cu = np.bincount(u, minlength=U)
        assert np.array_equal(cu[S.row_ids(len(lu))], lu) and cu.sum() == B and U > u.max(), name
        ent = i if pointwise else np.concatenate([i, j])
        ci = np.bincount(ent, minlength=I)
        assert np.array_equal(ci[S.row_ids(len(li))], li) and ci.sum() == E and I > ent.max(), name
        assert cu[2::3].sum() == 0 and ci[2::3].sum() == 0                  # every third row stays untouched
        if pointwise:
            assert set(np.unique(j)) <= {0, 1}
        elif len(li) > 1 and max(li) <= E // 4:
            assert (i == j).mean() <= max(li) / B, name       # (the exchange took the avoidable i == j away, or nearly)


ORACLE_CASES = ["one|one", "ones|ones", "period(16,1)|period(16,1)", "period(256,255)|period(256,255)",
                "comb(1,7)|comb(1,7)", "long(3)|long(3)"]


@pytest.mark.parametrize("d", [7, 64, 300])
@pytest.mark.parametrize("loss", [S.HL, S.SL])
def test_exact_step_is_the_oracle_bit_for_bit(d, loss):
    """ties the int64 reference to oracle.bpr_mf_numpy.mf_sgd_step (fp64, rounded once): loss and both tables"""
    B = 512
    E = B if loss == S.SL else 2 * B
    for k, name in enumerate(ORACLE_CASES):
        nu, ni = name.split("|")
        u, i, j, P, Q, _, st = S.make_case((name, S.named(B, nu), S.named(E, ni)), d, loss, seed=100 * d + k)
        S.assert_exact_domain(st)
        want_loss, Pn, Qn = O.mf_sgd_step(P, Q, u, i, j, S.LR[loss], 0.0, 0.0, loss_type=loss)
        assert float(st.loss) == want_loss, (name, st.loss, want_loss)
        assert np.array_equal(st.P_new().numpy(), Pn) and np.array_equal(st.Q_new().numpy(), Qn), name
        # the compact form the GPU test compares with
        Pc, Qc = P.copy(), Q.copy()
        Pc[st.urows.numpy()], Qc[st.irows.numpy()] = st.P_rows_new().numpy(), st.Q_rows_new().numpy()
        assert np.array_equal(Pc, Pn) and np.array_equal(Qc, Qn)
        # the raw gradients are the oracle's too
        grad = O.mf_point_grad if loss == S.SL else O.mf_pair_grad
        _, gP, gQ = grad(P, Q, u, i, j, 0.0, 0.0, loss_type=loss)
        assert np.array_equal(st.dense(st.urows, st.gP, P.shape[0]).numpy(), gP)
        assert np.array_equal(st.dense(st.irows, st.gQ, Q.shape[0]).numpy(), gQ)
        assert (Pn != P).any() or name == "one|one"


def test_exact_step_with_biases_is_the_fm_oracle():
    from oracle import fm_numpy as F
    B, d = 256, 20
    for k, name in enumerate(ORACLE_CASES):
        nu, ni = name.split("|")
        u, i, j, P, Q, b, st = S.make_case((name, S.named(B, nu), S.named(2 * B, ni)), d, S.HL, seed=k, biases=True)
        S.assert_exact_domain(st)
        want_loss, Pn, Qn, bun, bin_, b0n = F.fm_sgd_step(P, Q, *b, u, i, j, S.LR[S.HL], 0.0, 0.0, loss_type=S.HL)
        assert float(st.loss) == want_loss and np.array_equal(st.P_new().numpy(), Pn) and np.array_equal(st.Q_new().numpy(), Qn), name
        gb = st.dense(st.irows, st.g_i_bias, Q.shape[0]).numpy()
        assert np.array_equal((b[1].astype(np.float64) - S.LR[S.HL] * gb).astype(np.float32), np.asarray(bin_).reshape(-1)), name


def _gpu_case_families():
    """(id, cases, ds, loss, biases) of everything the GPU test runs"""
    fams = [("main-HL", S.main_cases(False), S.D_ALL, S.HL, False), ("main-HL-bias", S.main_cases(False), S.D_ALL, S.HL, True),
            ("main-SL", S.main_cases(True), S.D_SL, S.SL, False), ("long", S.long_cases(), S.D_LONG, S.HL, False)]
    fams += [(f"small-{B}", S.small_cases(B), S.D_ALL, S.HL, False) for B in S.B_SMALL]
    fams += [(f"off-grid-{B}", S.off_grid_cases(B), S.D_OFF_GRID, S.HL, False) for B in S.OFF_GRID]
    return fams


@pytest.mark.parametrize("fam,d", [(f, d) for f in _gpu_case_families() for d in f[2]], ids=lambda x: x[0] if isinstance(x, tuple) else str(x))
def test_domain_guard_holds_for_every_gpu_case(fam, d):
    """every (layout, d) of the GPU test (which checks its own cases once more before it runs them)"""
    _, cases, _, loss, biases = fam
    for k, case in enumerate(cases):
        S.assert_exact_domain(S.make_case(case, d, loss, seed=k, biases=biases)[-1])


def test_domain_guard_rejects_oversized_inputs():
    case = ("one|one", [4096], [8192])
    u, i, j, P, Q, _, st = S.make_case(case, 64, S.HL, seed=0)
    S.assert_exact_domain(st)
    with pytest.raises(AssertionError, match="2\\^24"):                    # a row of 2^23 x 4: the update leaves fp32's integers
        S.assert_exact_domain(S.exact_step(P * (1 << 21), Q, u, i, j, S.HL, S.LR[S.HL]))
    with pytest.raises(AssertionError, match="power of two"):
        S.assert_exact_domain(S.exact_step(P, Q, u, i, j, S.HL, 0.1))
    with pytest.raises(AssertionError, match="not integer"):
        S.exact_step(P * 0.3, Q, u, i, j, S.HL, S.LR[S.HL])
    # the squared loss at a learning rate that is a power of two but too large for its coefficients' span
    u, i, j, P, Q, _, st = S.make_case(("one|one", [4096], [4096]), 257, S.SL, seed=0)
    S.assert_exact_domain(st)
    big = S.exact_step(P * 64, Q * 64, u, i, j, S.SL, S.LR[S.SL])
    with pytest.raises(AssertionError, match="2\\^24"):
        S.assert_exact_domain(big)
