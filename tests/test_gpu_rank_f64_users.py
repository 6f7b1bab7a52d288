"""ops.{ease,slim,knn,psvd}_full_rank_users (csrc/rank_full_f64.hip) against tests/rank_f64_oracle.py:
bit for bit against int64 arithmetic on integer operands, and bit for bit against the existing *_rank / slim_scores
kernels on real-valued ones.  Every test here fails without the feature (AttributeError)."""
import functools

import numpy as np
import pytest
import torch

import rank_f64_oracle as RO

pytestmark = pytest.mark.gpu
DEV = "cuda"
BUF = 512                       # kRfBuf (csrc/rank_f64_users.h): the candidate buffer's capacity
CHUNK = 256                     # kRfChunk: items per step
VARIANTS = ("ease", "slim-lds", "slim-global", "knn-lds", "knn-global", "userknn", "psvd")
NAN, INF = float("nan"), float("inf")


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _rows_of(D):
    """the CSR triple (ptr int64, col int32 ascending, val float32) of a dense matrix, on the device"""
    D = np.asarray(D)
    nz = D != 0
    ptr = np.zeros(D.shape[0] + 1, np.int64)
    ptr[1:] = np.cumsum(nz.sum(1))
    r, c = np.nonzero(nz)
    col, val = c.astype(np.int32), D[r, c].astype(np.float32)
    if col.size == 0:
        col, val = np.zeros(1, np.int32), np.zeros(1, np.float32)
    return _t(ptr), _t(col), _t(val)


def _cols_of(D):
    """the by-column triple (ptr over the columns, rows ascending within a column)"""
    return _rows_of(np.asarray(D).T)


class Case:
    """The operands of one scorer, dense on the host (float64) and in the entry's form on the device.  left [U, inner],
    right [inner, I]: the score matrix is left @ right (PureSVD: right = item_vec^T)."""

    def __init__(self, variant, left, right):
        self.variant, self.kind = variant, "knn" if variant == "userknn" else variant.split("-")[0]
        self.path = variant.split("-")[1] if "-" in variant else "auto"
        self.left, self.right = np.asarray(left, np.float64), np.asarray(right, np.float64)
        self.U, self.I = self.left.shape[0], self.right.shape[1]
        if self.kind == "ease":
            self.dev = (_rows_of(self.left), _t(self.right))
        elif self.kind == "psvd":
            self.dev = (_t(self.left), _t(self.right.T))
        else:
            self.dev = (_rows_of(self.left), _cols_of(self.right))
        self.score_dtype = np.float32 if self.kind == "slim" else np.float64

    def run(self, users, topk, exclude=None, validate=True, return_scores=True):
        from daisyrec_amd import ops
        ex = None if exclude is None else tuple(_t(x) for x in exclude)
        users = _t(np.asarray(users, np.int64))
        kw = dict(exclude=ex, return_scores=return_scores, validate=validate)
        a, b = self.dev
        if self.kind == "ease":
            out = ops.ease_full_rank_users(a, b, users, topk, **kw)
        elif self.kind == "psvd":
            out = ops.psvd_full_rank_users(a, b, users, topk, **kw)
        elif self.kind == "slim":
            out = ops.slim_full_rank_users(a, b, self.I, users, topk, path=self.path, **kw)
        else:
            out = ops.knn_full_rank_users(a, b, self.left.shape[1], self.I, users, topk, path=self.path, **kw)
        if not return_scores:
            assert out.is_cuda and out.dtype == torch.int64
            return out.cpu().numpy()
        ids, scores = out
        assert ids.is_cuda and ids.dtype == torch.int64 and ids.shape == (len(users), topk) and scores.shape == ids.shape
        assert scores.dtype == (torch.float32 if self.kind == "slim" else torch.float64)
        return ids.cpu().numpy(), scores.cpu().numpy()

    def parent_scores(self, users, topk=0):
        """(scores [n, I], ids or None) of the EXISTING all-item path: the kernels this change does not touch"""
        from daisyrec_amd import ops
        users = _t(np.asarray(users, np.int64))
        a, b = self.dev
        if self.kind == "ease":
            s, ids = ops.ease_rank(a, b, users, None, topk)
        elif self.kind == "psvd":
            s, ids = ops.psvd_rank(a, b, users, None, topk)
        elif self.kind == "slim":
            s, ids = ops.slim_scores(a, b, self.I, users, None, path=self.path), None
        else:
            s, ids = ops.knn_rank(a, b, self.left.shape[1], self.I, users, None, topk, path=self.path)
        return s.cpu().numpy(), None if ids is None else ids.cpu().numpy()

    def exact_scores(self, users):
        """int64 arithmetic: every operand is an integer and every partial sum is far below 2^24"""
        Li, Ri = np.rint(self.left).astype(np.int64), np.rint(self.right).astype(np.int64)
        assert np.array_equal(Li, self.left) and np.array_equal(Ri, self.right)
        s = Li[np.asarray(users)] @ Ri
        assert np.abs(s).max(initial=0) < 2 ** 24
        return s.astype(self.score_dtype)


def _sparse_ints(rng, shape, density, lo=-8, hi=8):
    return rng.integers(lo, hi + 1, size=shape) * (rng.random(shape) < density)


def _make(variant, rng, U, I, ints=True):
    """operands of the variant over U users and I items: integers in [-8, 8] (a row of at most 700 entries keeps every sum
    below 2^16), or N(0, 1) values"""
    kind = variant.split("-")[0]
    val = (lambda shape, dens: _sparse_ints(rng, shape, dens)) if ints else \
        (lambda shape, dens: rng.standard_normal(shape).astype(np.float32) * (rng.random(shape) < dens))
    if kind == "psvd":
        k = 7
        dense = (lambda shape: rng.integers(-8, 9, size=shape)) if ints else (lambda shape: rng.standard_normal(shape))
        return Case(variant, dense((U, k)), dense((k, I)))
    if kind == "userknn":                       # L = the user similarity by row, R = X by column
        S, X = val((U, U), 0.3), val((U, I), 0.3)
        X[:, I // 2] = 0                        # an item nobody rated
        return Case(variant, S, X)
    X = val((U, I), 0.3)
    X[min(1, U - 1)] = 0                        # a user without history: every score is +0.0
    W = val((I, I), 1.0 if kind == "ease" else 0.1)
    return Case(variant, X, W)


def _random_exclusion(rng, U, I, share=0.2):
    return RO.user_csr({u: rng.choice(I, size=int(rng.integers(0, max(1, int(I * share)) + 1)), replace=False).tolist()
                        for u in range(U)}, U)


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _assert_same(got, want, what):
    (gi, gs), (wi, ws) = got, want
    assert np.array_equal(gi, wi), (what, "ids")
    assert gs.dtype == ws.dtype and np.array_equal(_bits(gs), _bits(ws)), (what, "score bits")


# ---- exact ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I", [1, 255, 256, 257, 700])
@pytest.mark.parametrize("variant", VARIANTS)
def test_exact_against_int64_arithmetic(variant, I):
    rng = np.random.default_rng(1000 + I)
    U = 40
    case = _make(variant, rng, U, I)
    excl = _random_exclusion(rng, U, I)
    for n in (1, 3, 70):
        users = rng.integers(0, U, size=n)                      # unsorted, with duplicates at n = 70
        if n == 70:
            users[:2] = (min(1, U - 1), min(1, U - 1))
        s = case.exact_scores(users)
        for topk in (1, 10, 50, 128):                           # 10, 50 and 128 are above I = 1; 128 is above 1 and 128 <= 255
            for ex in (None, excl):
                want = RO.rank_lists(s, topk, users=users, exclude=ex)
                _assert_same(case.run(users, topk, exclude=ex), want, (variant, I, n, topk, ex is not None))
    ids = case.run([0, 2 % U], 10, return_scores=False)
    assert np.array_equal(ids, RO.rank_lists(case.exact_scores([0, 2 % U]), 10)[0])


@pytest.mark.parametrize("variant", VARIANTS)
def test_topk_above_the_item_count(variant):
    rng = np.random.default_rng(3)
    U, I = 9, 100
    case = _make(variant, rng, U, I)
    users = [8, 0, 1, 8]
    excl = _random_exclusion(rng, U, I)
    ids, sc = case.run(users, 128, exclude=excl)
    _assert_same((ids, sc), RO.rank_lists(case.exact_scores(users), 128, users=users, exclude=excl), variant)
    assert (ids[:, I:] == -1).all() and np.isneginf(sc[:, I:]).all() and (ids[:, 0] >= 0).all()


# ---- the same bits as the existing kernels --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _real_case(variant):
    rng = np.random.default_rng(77)
    U, I = 300, 700
    case = _make(variant, rng, U, I, ints=False)
    users = rng.permutation(U)
    scores, _ = case.parent_scores(users)
    scores.setflags(write=False)
    return case, users, scores, _random_exclusion(rng, U, I)


@pytest.mark.parametrize("variant", VARIANTS)
def test_same_bits_as_the_existing_rank_path(variant):
    case, users, scores, excl = _real_case(variant)
    assert scores.shape == (300, 700) and scores.dtype == case.score_dtype and np.isfinite(scores).all()
    for topk in (10, 128):
        got = case.run(users, topk, exclude=excl)
        _assert_same(got, RO.rank_lists(scores, topk, users=users, exclude=excl), (variant, topk, "excluded"))
        got = case.run(users, topk)
        _assert_same(got, RO.rank_lists(scores, topk), (variant, topk))
        _, parent_ids = case.parent_scores(users, topk)
        if parent_ids is not None:                              # (slim_scores selects nothing itself)
            assert np.array_equal(got[0], parent_ids), (variant, topk, "the existing top-k")


@pytest.mark.parametrize("variant", VARIANTS)
def test_two_calls_give_the_same_bits(variant):
    case, users, _, excl = _real_case(variant)
    a, b = case.run(users, 50, exclude=excl), case.run(users, 50, exclude=excl)
    _assert_same(a, b, variant)


def test_torch_library_ops_call_the_same_entries():
    """torch.ops.daisyrec.*_full_rank_users (csrc/torch_ops.cpp) against the ctypes route, with and without exclusion"""
    import daisyrec_amd.torch_ops  # noqa: F401
    T = torch.ops.daisyrec
    for variant in ("ease", "slim-lds", "knn-lds", "userknn", "psvd"):
        case, users, _, excl = _real_case(variant)
        us, ex = _t(np.asarray(users[:40], np.int64)), tuple(_t(x) for x in excl)
        a, b = case.dev
        for e in ((None, None), ex):
            if case.kind == "ease":
                ids, sc = T.ease_full_rank_users(*a, b, us, e[0], e[1], 20)
            elif case.kind == "psvd":
                ids, sc = T.psvd_full_rank_users(a, b, us, e[0], e[1], 20)
            elif case.kind == "slim":
                ids, sc = T.slim_full_rank_users(*a, *b, us, e[0], e[1], 20)
            else:
                ids, sc = T.knn_full_rank_users(*a, case.left.shape[1], *b, us, e[0], e[1], 20)
            want = case.run(users[:40], 20, exclude=None if e[0] is None else excl)
            _assert_same((ids.cpu().numpy(), sc.cpu().numpy()), want, variant)
    case = _real_case("psvd")[0]
    with pytest.raises(RuntimeError, match="cap of 128"):
        T.psvd_full_rank_users(*case.dev, _t(np.zeros(1, np.int64)), None, None, 129)
    with pytest.raises(RuntimeError, match="together"):
        T.psvd_full_rank_users(*case.dev, _t(np.zeros(1, np.int64)), _t(np.zeros(301, np.int64)), None, 5)


# ---- the selector ---------------------------------------------------------------------------------------------------------------
def _psvd_with_scores(rows):
    """a PureSVD case whose score matrix is `rows` [U, I] exactly: user_vec = the identity, item_vec^T = rows"""
    rows = np.asarray(rows, np.float64)
    return Case("psvd", np.eye(rows.shape[0]), rows)


def test_rising_falling_and_equal_scores():
    I = 2 * BUF + CHUNK + 37                                    # the buffer is compacted after every chunk but the first
    up = np.arange(I, dtype=np.float64) - 400.0                 # every item beats the threshold
    down = -up                                                  # nothing is appended after the first chunk
    flat = np.zeros(I)                                          # every score equal: ids in ascending order
    case = _psvd_with_scores(np.stack([up, down, flat, flat]))
    users = [0, 1, 2, 3, 0]
    excl = RO.user_csr({0: [I - 1, I - 3], 1: [0, 2], 3: [0, 1, 5, CHUNK - 1, CHUNK, I - 1]}, 4)
    s = case.exact_scores(users).astype(np.float64)
    for topk in (1, 50, 128):
        for ex in (None, excl):
            _assert_same(case.run(users, topk, exclude=ex), RO.rank_lists(s, topk, users=users, exclude=ex), (topk, ex is not None))
    ids, _ = case.run([3], 8, exclude=excl)
    assert ids.tolist() == [[2, 3, 4, 6, 7, 8, 9, 10]]
    # the other scorers see equal scores through a user without history (+0.0 everywhere)
    rng = np.random.default_rng(5)
    for variant in ("ease", "slim-lds", "slim-global", "knn-lds", "knn-global"):
        c = _make(variant, rng, 4, 300)
        ids, sc = c.run([1], 6, exclude=RO.user_csr({1: [0, 3]}, 4))
        assert ids.tolist() == [[1, 2, 4, 5, 6, 7]] and not sc.any() and not np.signbit(sc).any(), variant


def test_exactly_topk_and_one_fewer_eligible_items():
    I, topk = 600, 50
    rng = np.random.default_rng(6)
    case = _psvd_with_scores(rng.integers(-8, 9, size=(3, I)))
    keep_k = sorted(rng.choice(I, size=topk, replace=False).tolist())
    keep_k1 = keep_k[:-1]
    excl = RO.user_csr({0: sorted(set(range(I)) - set(keep_k)), 1: sorted(set(range(I)) - set(keep_k1))}, 3)
    users = [1, 0, 2]
    ids, sc = case.run(users, topk, exclude=excl)
    _assert_same((ids, sc), RO.rank_lists(case.exact_scores(users).astype(np.float64), topk, users=users, exclude=excl), "")
    assert sorted(ids[1].tolist()) == keep_k
    assert sorted(ids[0, :-1].tolist()) == keep_k1 and ids[0, -1] == -1 and np.isneginf(sc[0, -1])


@pytest.mark.parametrize("variant", ["psvd", "ease"])
def test_nan_is_never_selected_and_inf_ranks_first(variant):
    rng = np.random.default_rng(8)
    U, I = 6, 300
    case = _make(variant, rng, U, I)
    if variant == "psvd":                                       # a factor of user_vec: NaN poisons user 2's every score,
        case.left[2, 3] = NAN                                   # +inf gives user 4 scores of +inf, -inf and NaN (inf * 0)
        case.left[4, 0] = INF
        case = Case(variant, case.left, case.right)
    else:                                                       # an entry of W: one column of some users' scores
        case.left[:, 7] = np.where(np.arange(U) % 2 == 0, 1.0, case.left[:, 7])
        case.left[:, 9] = np.where(np.arange(U) % 2 == 0, 2.0, case.left[:, 9])
        case.right[7, 100] = NAN
        case.right[9, 200] = INF
        case = Case(variant, case.left, case.right)
    users = np.arange(U)
    scores, _ = case.parent_scores(users)                       # IEEE arithmetic on the device: the existing kernel's
    assert np.isnan(scores).any() and np.isposinf(scores).any()
    for topk in (5, 128):
        got = case.run(users, topk)
        _assert_same(got, RO.rank_lists(scores, topk), (variant, topk))
        picked = np.take_along_axis(scores, np.maximum(got[0], 0), 1)[got[0] >= 0]
        assert not np.isnan(picked).any()
    if variant == "psvd":
        assert (case.run([2], 5)[0] == -1).all()                # nothing comparable
    else:
        assert case.run([0], 5)[0][0, 0] == 200 and 100 not in case.run([0], 128)[0]


# ---- the exclusion ---------------------------------------------------------------------------------------------------------------
def test_exclusion_edges():
    rng = np.random.default_rng(9)
    U, I = 8, 700
    for variant in ("psvd", "knn-global"):
        case = _make(variant, rng, U, I)
        rows = {0: [], 1: list(range(I)), 2: [0, 0, 5, 5, 5, CHUNK - 1, CHUNK, CHUNK, 2 * CHUNK - 1, 2 * CHUNK, I - 1, I - 1],
                3: [CHUNK - 1, I - 1, I, I + 7, 2 ** 31 - 1], 4: [0], 5: [I - 1], 6: list(range(0, I, 2)),
                7: list(range(CHUNK, 2 * CHUNK))}
        indptr = np.zeros(U + 1, np.int64)
        indptr[1:] = np.cumsum([len(rows[u]) for u in range(U)])
        excl = (indptr, np.array([i for u in range(U) for i in rows[u]], np.int32))
        users = [7, 1, 0, 2, 3, 3, 6, 5, 4]
        s = case.exact_scores(users)
        for topk in (3, 128):
            got = case.run(users, topk, exclude=excl)
            _assert_same(got, RO.rank_lists(s, topk, users=users, exclude=excl), (variant, topk))
            assert (got[0][1] == -1).all() and np.isneginf(got[1][1]).all()         # every item excluded


def test_unsorted_rows_and_bad_user_ids():
    rng = np.random.default_rng(10)
    U, I = 5, 600
    case = _make("psvd", rng, U, I)
    row = rng.permutation(I)[:400].astype(np.int32)
    assert (np.diff(row) < 0).any()
    indptr = np.array([0, 0, 400, 400, 400, 400], np.int64)
    with pytest.raises(ValueError, match="ascending"):
        case.run([1], 20, exclude=(indptr, row))
    ids, sc = case.run([1, 0, 1], 128, exclude=(indptr, row), validate=False)
    assert ((ids >= -1) & (ids < I)).all()
    for r in ids:
        kept = r[r >= 0]
        assert len(set(kept.tolist())) == kept.size             # no id repeats within a list
    _assert_same((ids[1:2], sc[1:2]), RO.rank_lists(case.exact_scores([0]).astype(np.float64), 128), "the row without exclusion")
    for bad in ([0, U], [-1]):
        with pytest.raises(IndexError):
            case.run(bad, 5)
    with pytest.raises(ValueError, match="cap of 128"):
        case.run([0], 129)
    with pytest.raises(ValueError):
        case.run([0], 0)
    short = (np.zeros(U, np.int64), np.zeros(1, np.int32))
    with pytest.raises(ValueError, match="indptr"):
        case.run([0], 5, exclude=short)
    ids, sc = case.run(np.zeros(0, np.int64), 5)
    assert ids.shape == (0, 5) and sc.shape == (0, 5)
