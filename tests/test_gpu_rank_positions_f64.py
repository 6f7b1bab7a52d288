"""ops.{ease,slim,knn,psvd}_full_rank_positions (csrc/rank_positions_f64.hip) against
tests/rank_positions_f64_oracle.py: positions, score bits and eligible counts exactly against int64 arithmetic on integer
operands, and on real-valued ones against the existing kernels' scores and the lists of *_full_rank_users.  Every test
here fails without the feature (AttributeError)."""
import numpy as np
import pytest
import torch

import rank_f64_oracle as RO
import rank_positions_f64_oracle as PO
from test_gpu_rank_f64_users import NAN, INF, VARIANTS, Case, _bits, _make, _random_exclusion, _real_case, _t

pytestmark = pytest.mark.gpu
TC = 512                        # kRcTc (csrc/rank_count.h): targets a workgroup ranks per pass over the items
FEW = 16                        # kRcFew: blocks of fewer ranked targets count bucket by bucket


def run_pos(case, users, targets, exclude=None, validate=True, return_scores=True, return_eligible=True):
    """the entry of the case's variant -> numpy (out_indptr, pos[, scores][, eligible])"""
    from daisyrec_amd import ops
    assert TC == ops.RANK_COUNT_BLOCK
    ex = None if exclude is None else tuple(_t(x) for x in exclude)
    tg = tuple(_t(x) for x in targets)
    us = _t(np.asarray(users, np.int64))
    kw = dict(exclude=ex, return_scores=return_scores, return_eligible=return_eligible, validate=validate)
    a, b = case.dev
    if case.kind == "ease":
        out = ops.ease_full_rank_positions(a, b, us, tg, **kw)
    elif case.kind == "psvd":
        out = ops.psvd_full_rank_positions(a, b, us, tg, **kw)
    elif case.kind == "slim":
        out = ops.slim_full_rank_positions(a, b, case.I, us, tg, path=case.path, **kw)
    else:
        out = ops.knn_full_rank_positions(a, b, case.left.shape[1], case.I, us, tg, path=case.path, **kw)
    assert len(out) == 2 + return_scores + return_eligible and all(t.is_cuda for t in out)
    assert out[0].dtype == torch.int64 and out[0].shape == (len(users) + 1,) and out[1].dtype == torch.int32
    if return_scores:
        assert out[2].dtype == (torch.float32 if case.kind == "slim" else torch.float64) and out[2].shape == out[1].shape
    if return_eligible:
        assert out[-1].dtype == torch.int32 and out[-1].shape == (len(users),)
    return tuple(t.cpu().numpy() for t in out)


def _assert_same(got, want, what):
    (gp, gpos, gs, ge), (wp, wpos, ws, we) = got, want
    assert np.array_equal(gp, wp), (what, "out_indptr")
    assert np.array_equal(gpos, wpos), (what, "positions", np.nonzero(gpos != wpos)[0][:8], gpos[gpos != wpos][:8], wpos[gpos != wpos][:8])
    assert gs.dtype == ws.dtype and np.array_equal(_bits(gs), _bits(ws)), (what, "score bits")
    assert np.array_equal(ge, we), (what, "eligible")


def _target_csr(rng, U, I, lengths):
    """a target CSR over U users: user u < len(lengths) gets min(lengths[u], I) items, the others 0 .. 10; rows ascending"""
    rows = {}
    for u in range(U):
        k = min(lengths[u], I) if u < len(lengths) else int(rng.integers(0, min(I, 10) + 1))
        rows[u] = rng.choice(I, size=k, replace=False).tolist()
    return RO.user_csr(rows, U)


# ---- exact ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I", [1, 255, 256, 257, 700, 2 * TC + 37])
@pytest.mark.parametrize("variant", VARIANTS)
def test_exact_against_int64_arithmetic(variant, I):
    rng = np.random.default_rng(2000 + I)
    U = 40
    case = _make(variant, rng, U, I)
    # rows of 0, 1, Tc - 1, Tc, Tc + 1 and I targets (user 1 is the one without history), as far as I allows; I = 2 Tc + 37
    # walks the block loop three times; 15, 16 and 17 targets: around FEW, where the bucket additions change their form
    targets = _target_csr(rng, U, I, [0, 1, TC - 1, TC, TC + 1, I, FEW - 1, FEW, FEW + 1])
    excl = _random_exclusion(rng, U, I)                         # overlaps the long rows for certain
    draws = ([5], [4, 0, 3], np.concatenate([[1, 1, 5, 2, 0, 3, 4, 5, 8, 6, 7], rng.integers(0, U, size=59)]))
    for users in draws:                                         # n = 1, 3 and 70: unsorted, with duplicates
        users = np.asarray(users)
        s = case.exact_scores(users)
        rows = PO.target_rows(targets, users)
        for ex in (None, excl):
            want = PO.positions(s, rows, users=users, exclude=ex)
            _assert_same(run_pos(case, users, targets, exclude=ex), want, (variant, I, len(users), ex is not None))
    # the optional outputs alone
    users = np.asarray(draws[1])
    want = PO.positions(case.exact_scores(users), PO.target_rows(targets, users), users=users, exclude=excl)
    p, pos = run_pos(case, users, targets, exclude=excl, return_scores=False, return_eligible=False)
    assert np.array_equal(p, want[0]) and np.array_equal(pos, want[1])
    p, pos, el = run_pos(case, users, targets, exclude=excl, return_scores=False)
    assert np.array_equal(pos, want[1]) and np.array_equal(el, want[3])


@pytest.mark.parametrize("variant", ["ease", "slim-lds", "slim-global", "knn-lds", "knn-global"])
def test_a_user_without_history_ranks_by_id(variant):
    rng = np.random.default_rng(5)
    U, I = 4, 300
    case = _make(variant, rng, U, I)                            # user 1: every score is +0.0
    targets = RO.user_csr({1: [0, 1, 2, 3, 4, 150, 298, 299], 2: [7]}, U)
    excl = RO.user_csr({1: [0, 3, 200]}, U)
    _, pos, sc, el = run_pos(case, [1], targets, exclude=excl)
    assert pos.tolist() == [-1, 0, 1, -1, 2, 148, 295, 296] and el.tolist() == [I - 3]
    assert np.isneginf(sc[[0, 3]]).all() and not sc[[1, 2, 4, 5, 6, 7]].any() and not np.signbit(sc[[1, 2, 4, 5, 6, 7]]).any()
    _, pos, el = run_pos(case, [1, 1], targets, return_scores=False)
    assert pos.tolist() == [0, 1, 2, 3, 4, 150, 298, 299] * 2 and el.tolist() == [I, I]


@pytest.mark.parametrize("variant", ["psvd", "slim-global", "userknn"])
def test_bad_targets_give_minus_one_without_validation(variant):
    rng = np.random.default_rng(12)
    U, I = 6, 600
    case = _make(variant, rng, U, I)
    indptr = np.array([0, 0, 0, 8, 8, 8, 11], np.int64)       # user 2: out of range, negative, excluded, unsorted, repeated
    items = np.array([I, -1, 17, 5, -2 ** 31, 2 ** 31 - 1, 5, I + 7, 3, 2, 1], np.int32)
    excl = RO.user_csr({2: [17, 90], 5: [2]}, U)
    users = [2, 5, 0, 2]
    with pytest.raises(ValueError, match="ascending"):
        run_pos(case, users, (indptr, items), exclude=excl)
    got = run_pos(case, users, (indptr, items), exclude=excl, validate=False)
    want = PO.positions(case.exact_scores(users), PO.target_rows((indptr, items), users), users=users, exclude=excl)
    _assert_same(got, want, variant)
    assert (got[1][[0, 1, 2, 4, 5, 7]] == -1).all() and np.isneginf(got[2][[0, 1, 2, 4, 5, 7]]).all()
    assert got[1][3] == got[1][6] >= 0 and got[1][9] == -1 and (got[1][[8, 10]] >= 0).all()


@pytest.mark.parametrize("variant", ["psvd", "ease"])
def test_nan_is_never_ranked_and_inf_ranks_first(variant):
    """the constructions of test_gpu_rank_f64_users.test_nan_is_never_selected_and_inf_ranks_first"""
    rng = np.random.default_rng(8)
    U, I = 6, 300
    case = _make(variant, rng, U, I)
    if variant == "psvd":                                       # a factor of user_vec: NaN poisons user 2's every score,
        case.left[2, 3] = NAN                                   # +inf gives user 4 scores of +inf, -inf and NaN (inf * 0)
        case.left[4, 0] = INF
    else:                                                       # an entry of W: one column of some users' scores
        case.left[:, 7] = np.where(np.arange(U) % 2 == 0, 1.0, case.left[:, 7])
        case.left[:, 9] = np.where(np.arange(U) % 2 == 0, 2.0, case.left[:, 9])
        case.right[7, 100] = NAN
        case.right[9, 200] = INF
    case = Case(variant, case.left, case.right)
    users = np.arange(U)
    scores, _ = case.parent_scores(users)                       # IEEE arithmetic on the device: the existing kernel's
    assert np.isnan(scores).any() and np.isposinf(scores).any()
    targets = RO.user_csr({u: range(I) for u in range(U)}, U)   # every item of every user
    excl = _random_exclusion(rng, U, I)
    for ex in (None, excl):
        got = run_pos(case, users, targets, exclude=ex)
        _assert_same(got, PO.positions(scores, PO.target_rows(targets, users), users=users, exclude=ex), (variant, ex is not None))
    _, pos, sc, el = run_pos(case, users, targets)
    pos, sc = pos.reshape(U, I), sc.reshape(U, I)
    assert (pos[np.isnan(scores)] == -1).all() and np.isnan(sc[np.isnan(scores)]).all()     # the NaN itself comes back
    assert np.array_equal(el, (~np.isnan(scores)).sum(1))       # NaN items are not eligible ...
    for u in range(U):                                          # ... and not counted: the ranked positions are 0 .. eligible - 1
        assert sorted(pos[u][pos[u] >= 0].tolist()) == list(range(el[u]))
    if variant == "psvd":
        assert el[2] == 0 and (pos[2] == -1).all()              # nothing comparable
        first = np.nonzero(np.isposinf(scores[4]))[0]
        assert sorted(pos[4, first].tolist()) == list(range(first.size))
    else:
        assert pos[0, 200] == 0 and pos[0, 100] == -1


# ---- real values: the existing kernels' bits and lists ----------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_real_values_against_the_existing_kernels_and_lists(variant):
    case, users, scores, excl = _real_case(variant)             # 300 x 700; scores: the existing all-item kernels'
    U, I = case.U, case.I
    rng = np.random.default_rng(78)
    rows = {u: rng.choice(I, size=10, replace=False).tolist() for u in range(U)}
    rows[int(users[0])] = list(range(I))                        # one row longer than a block
    targets = RO.user_csr(rows, U)
    tr = PO.target_rows(targets, users)
    for ex in (None, excl):
        got = run_pos(case, users, targets, exclude=ex)
        want = PO.positions(scores, tr, users=users, exclude=ex)
        _assert_same(got, want, (variant, ex is not None))      # (score bits: parent_scores at the targets)
        again = run_pos(case, users, targets, exclude=ex)
        for a, b in zip(got, again):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (variant, "two calls")
        # the statement of the contract, against the list call with the same arguments
        ids, _ = case.run(users, 128, exclude=ex)
        out_indptr, pos = got[0], got[1]
        for b in range(len(users)):
            p = pos[out_indptr[b]:out_indptr[b + 1]]
            t = np.asarray(tr[b])
            listed = (p >= 0) & (p < 128)
            assert np.array_equal(ids[b][p[listed]], t[listed]), (variant, b)               # ids[b, pos] == t
            assert set(ids[b].tolist()) & set(t.tolist()) == set(t[listed].tolist()), (variant, b)   # and no other target
            assert got[3][b] >= (ids[b] >= 0).sum()
    assert (got[3] == I - np.array([len(set(excl[1][excl[0][u]:excl[0][u + 1]].tolist())) for u in users])).all()


def test_errors_and_the_empty_request():
    rng = np.random.default_rng(10)
    U, I = 5, 100
    case = _make("psvd", rng, U, I)
    targets = RO.user_csr({0: [1, 2], 3: [5]}, U)
    for bad in ([0, U], [-1]):
        with pytest.raises(IndexError):
            run_pos(case, bad, targets)
    with pytest.raises(ValueError, match="twice"):
        run_pos(case, [0], (np.array([0, 2, 2, 2, 2, 2], np.int64), np.array([4, 4], np.int32)))
    with pytest.raises(ValueError, match="indptr"):
        run_pos(case, [0], (np.zeros(U, np.int64), np.zeros(1, np.int32)))
    with pytest.raises(ValueError, match="indptr"):
        run_pos(case, [0], (np.zeros(U, np.int64), np.zeros(1, np.int32)), validate=False)
    p, pos, sc, el = run_pos(case, np.zeros(0, np.int64), targets)
    assert p.tolist() == [0] and pos.size == 0 and sc.size == 0 and el.size == 0
    p, pos, sc, el = run_pos(case, [1, 2], targets)             # requests without targets still count their eligible items
    assert p.tolist() == [0, 0, 0] and pos.size == 0 and el.tolist() == [I, I]
    empty = (np.zeros(U + 1, np.int64), np.zeros(0, np.int32))
    p, pos, el = run_pos(case, [4, 0], empty, exclude=RO.user_csr({4: [3, 3, 9]}, U), return_scores=False, validate=False)
    assert p.tolist() == [0, 0, 0] and el.tolist() == [I - 2, I]
