"""ops.rank_rows_f32 (csrc/rank_rows.hip) against tests/full_rank_oracle.py: ids AND score bytes are equal
for every size around the kernel's step, every row layout (pitch, alignment: the float4 and the element loads), every
kind of row content and every exclusion case.  Every test here fails without the feature (AttributeError)."""
import numpy as np
import pytest
import torch

import full_rank_oracle as FO

pytestmark = pytest.mark.gpu
U = 9                   # rows of the exclusion CSR


def _step():
    from daisyrec_amd import ops
    return ops.RANK_ROWS_STEP


def _csr(rows):
    """(indptr int64 [U + 1], items int32) device tensors and the numpy pair, from a list of U arrays"""
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    items = np.concatenate([np.asarray(r, np.int32) for r in rows]) if indptr[-1] else np.zeros(0, np.int32)
    return (torch.from_numpy(indptr).cuda(), torch.from_numpy(items).cuda()), (indptr, items)


def _random_rows(rng, I, frac):
    return [np.sort(rng.choice(I, int(round(frac * I)), replace=False)) for _ in range(U)]


def _check(t, topk, row_users=None, rows=None, validate=True):
    """t: a 2-D device tensor (any view).  ids and score bytes against the oracle on t's own values."""
    from daisyrec_amd import ops
    s = t.cpu().numpy()
    m, I = s.shape
    dev = host = None
    if rows is not None:
        dev, host = _csr(rows)
    ru = list(range(m)) if row_users is None else list(row_users)
    want_ids, want_sc = FO.rank_lists(s, FO.exclusion_sets(host, ru), min(topk, I))
    ids, sc = ops.rank_rows_f32(t, topk, row_users=None if rows is None else torch.tensor(ru), exclude=dev,
                                return_scores=True, validate=validate)
    assert ids.is_cuda and ids.dtype == torch.int64 and ids.shape == want_ids.shape and sc.dtype == torch.float32
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    assert np.array_equal(ids, want_ids), (I, m, topk, np.argwhere(ids != want_ids)[:4])
    assert np.array_equal(sc.view(np.uint32), want_sc.view(np.uint32)), (I, m, topk)
    ids_only = ops.rank_rows_f32(t, topk, row_users=None if rows is None else torch.tensor(ru), exclude=dev)
    assert np.array_equal(ids_only.cpu().numpy(), want_ids)
    return ids, sc


def _sizes():
    S = _step()
    return [1, S - 1, S, S + 1, 3 * S + 7]


@pytest.mark.parametrize("k", range(5))
def test_sizes_around_the_step(k):
    I = _sizes()[k]
    rng = np.random.default_rng(100 + I)
    for m in (1, 5):
        t = torch.from_numpy(rng.standard_normal((m, I)).astype(np.float32)).cuda()
        rows = _random_rows(rng, I, 0.2)
        users = rng.integers(0, U, m)
        for topk in (1, 10, 128) + ((I,) if I < 128 else ()):
            _check(t, topk)
            _check(t, topk, users, rows)


def test_row_layouts():
    """pitch > I, rows that are not 16-byte aligned, a misaligned first element: every combination takes the float4 or the
    element loads, chosen per launch, and gives the same lists"""
    from daisyrec_amd import ops
    S = _step()
    rng = np.random.default_rng(7)
    m = 5
    for I in (S + 1, 2 * S + 4, 2 * S + 5, 777):
        pitch = I + 8 + (-I) % 4                                # a multiple of 4: aligned views take the float4 loads,
        big = torch.from_numpy(rng.standard_normal((m, pitch)).astype(np.float32)).cuda()      # I % 4 != 0 leaves a tail
        rows = _random_rows(rng, I, 0.2)
        users = rng.integers(0, U, m)
        for view in (big[:, :I], big[:, 4:4 + I]):              # the second starts 16 bytes in
            assert view.stride(0) == pitch and view.data_ptr() % 16 == 0
            _check(view, 10, users, rows)
        _check(big[:, 1:1 + I], 10, users, rows)                # first element 4 bytes past a 16-byte boundary
        tight = big[:, :I].contiguous()                         # pitch == I: odd I -> rows not 16-byte aligned
        _check(tight, 128, users, rows)
        flat = torch.zeros(m * I + 3, dtype=torch.float32, device="cuda")
        flat[1:1 + m * I] = tight.reshape(-1)
        shifted = flat[1:1 + m * I].view(m, I)                  # contiguous, first element not 16-byte aligned
        assert shifted.data_ptr() % 16 != 0
        a = ops.rank_rows_f32(shifted, 10, return_scores=True)
        b = ops.rank_rows_f32(tight, 10, return_scores=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        _check(shifted, 10, users, rows)
    one = big[2:3, :777]                                        # a single row: its stride does not matter
    _check(one, 10)


def _contents(rng, I):
    S = _step()
    spec = rng.standard_normal(I).astype(np.float32)
    spec[rng.choice(I, I // 3, replace=False)] = 0.0            # zeros of both signs tie with each other by id
    spec[rng.choice(I, I // 6, replace=False)] = -0.0
    at = rng.choice(I, min(I, 40), replace=False)
    spec[at] = np.resize(np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 0.0, -0.0, np.nan], np.float32), at.size)
    return {
        "small integers": rng.integers(-2, 3, I).astype(np.float32),
        "all equal": np.full(I, 1.5, np.float32),
        "rising": np.arange(I, dtype=np.float32),               # compacts at every step
        "falling": -np.arange(I, dtype=np.float32),             # never compacts after the first
        "specials": spec,
        "normals": rng.standard_normal(I).astype(np.float32),
        "all -inf": np.full(I, -np.inf, np.float32),
        "all nan": np.full(I, np.nan, np.float32),
        "late peak": np.where(np.arange(I) >= I - min(I, 130), 5.0, rng.standard_normal(I)).astype(np.float32) if I > S else
                     rng.standard_normal(I).astype(np.float32),
    }


@pytest.mark.parametrize("k", range(5))
def test_row_contents(k):
    I = _sizes()[k]
    rng = np.random.default_rng(900 + I)
    c = _contents(rng, I)
    t = torch.from_numpy(np.stack(list(c.values()))).cuda()
    rows = _random_rows(rng, I, 0.2)
    users = rng.integers(0, U, t.shape[0])
    for topk in (1, 10, 128):
        _check(t, topk)
        ids, sc = _check(t, topk, users, rows)
    nan_row = list(c).index("specials")
    if I > 128:
        assert np.isnan(sc[nan_row, 0])                          # a NaN ranks first


@pytest.mark.parametrize("I", [90, 1024 + 1, 3 * 1024 + 7])
def test_exclusion_cases(I):
    rng = np.random.default_rng(40 + I)
    topk = 10
    t = torch.from_numpy(np.stack([rng.standard_normal(I), rng.integers(-2, 3, I)]).astype(np.float32)).cuda()
    everything = np.arange(I)
    keep3 = np.sort(rng.choice(I, 3, replace=False))
    some = np.sort(rng.choice(I, I // 5, replace=False))
    rows = [np.zeros(0, np.int32),                                              # 0: nothing
            some,                                                               # 1: 20 %
            np.setdiff1d(everything, keep3),                                    # 2: everything but 3 items
            np.setdiff1d(everything, rng.choice(I, topk, replace=False)),       # 3: exactly topk eligible
            np.setdiff1d(everything, rng.choice(I, topk - 1, replace=False)),   # 4: topk - 1 eligible
            np.sort(np.concatenate([some, some[::3], some[:5]])),               # 5: duplicates
            everything,                                                         # 6: everything
            np.array([0, I - 1]), np.array([I - 1])]                            # 7, 8: the ends
    assert len(rows) == U
    for users in ([0, 1], [2, 3], [4, 5], [6, 7], [8, 2], [5, 5]):
        ids, sc = _check(t, topk, users, rows)
    ids, sc = _check(t, topk, [2, 4], rows)
    assert sorted(ids[0, :3].tolist()) == keep3.tolist() and np.all(ids[0, 3:] == -1) and np.all(np.isneginf(sc[0, 3:]))
    assert np.all(ids[1, :topk - 1] >= 0) and ids[1, topk - 1] == -1
    # more rows than CSR rows, unsorted, users repeated
    many = torch.from_numpy(rng.standard_normal((7, I)).astype(np.float32)).cuda()
    _check(many, topk, [8, 1, 5, 1, 0, 3, 1], rows)
    _check(many, 128 if I > 128 else I, [8, 1, 5, 1, 0, 3, 1], rows)


def test_rows_that_break_the_contract_cost_exclusions_only():
    """validate=False, an unsorted row and entries >= I or < 0: contents are only compared, so the ids stay in range and
    distinct and every list is full"""
    from daisyrec_amd import ops
    I, topk = 2 * _step() + 5, 10
    rng = np.random.default_rng(5)
    t = torch.from_numpy(rng.standard_normal((3, I)).astype(np.float32)).cuda()
    rows = [rng.permutation(I)[:700], np.array([I, I + 5, 2 ** 31 - 1, 3, -4, 1]), np.arange(50)[::-1].copy()] + \
           [np.zeros(0, np.int32)] * (U - 3)
    dev, _ = _csr(rows)
    ids, sc = ops.rank_rows_f32(t, topk, row_users=torch.tensor([0, 1, 2]), exclude=dev, return_scores=True, validate=False)
    ids, sc, s = ids.cpu().numpy(), sc.cpu().numpy(), t.cpu().numpy()
    for b in range(3):
        assert np.all((ids[b] >= 0) & (ids[b] < I)) and len(set(ids[b].tolist())) == topk
        assert np.array_equal(sc[b], s[b, ids[b]]) and np.all(sc[b, 1:] <= sc[b, :-1])


def test_two_calls_give_the_same_bits():
    from daisyrec_amd import ops
    I = 3 * _step() + 7
    rng = np.random.default_rng(11)
    t = torch.from_numpy(rng.integers(-3, 4, (40, I)).astype(np.float32)).cuda()
    dev, _ = _csr(_random_rows(rng, I, 0.3))
    users = torch.from_numpy(rng.integers(0, U, 40))
    a = ops.rank_rows_f32(t, 50, row_users=users, exclude=dev, return_scores=True)
    b = ops.rank_rows_f32(t, 50, row_users=users, exclude=dev, return_scores=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_the_torch_op_takes_the_same_route():
    import daisyrec_amd.torch_ops  # noqa: F401
    from daisyrec_amd import ops
    I = _step() + 9
    rng = np.random.default_rng(3)
    big = torch.from_numpy(rng.standard_normal((6, I + 3)).astype(np.float32)).cuda()
    (indptr, items), _ = _csr(_random_rows(rng, I, 0.2))
    users = torch.from_numpy(rng.integers(0, U, 6)).cuda()
    for t in (big[:, :I], big[:, :I].contiguous()):
        ids, sc = torch.ops.daisyrec.rank_rows_f32(t, users, indptr, items, 10)
        want = ops.rank_rows_f32(t, 10, row_users=users, exclude=(indptr, items), return_scores=True)
        assert torch.equal(ids, want[0]) and torch.equal(sc.view(torch.int32), want[1].view(torch.int32))
        ids, sc = torch.ops.daisyrec.rank_rows_f32(t, None, None, None, 10)
        assert torch.equal(ids, ops.rank_rows_f32(t, 10))
    with pytest.raises(RuntimeError, match="cap of 128"):
        torch.ops.daisyrec.rank_rows_f32(big, None, None, None, 129)
    with pytest.raises(RuntimeError, match="row_users"):
        torch.ops.daisyrec.rank_rows_f32(big, None, indptr, items, 10)


def test_validation_and_argument_errors():
    from daisyrec_amd import ops
    I = 300
    t = torch.zeros(2, I, device="cuda")
    dev, _ = _csr([np.arange(3)] * U)
    with pytest.raises(IndexError):
        ops.rank_rows_f32(t, 5, row_users=[0, U], exclude=dev)
    with pytest.raises(IndexError):
        ops.rank_rows_f32(t, 5, row_users=[-1, 0], exclude=dev)
    bad_rows, _ = _csr([np.array([9, 3])] + [np.zeros(0, np.int32)] * (U - 1))
    with pytest.raises(ValueError, match="ascending"):
        ops.rank_rows_f32(t, 5, row_users=[0, 1], exclude=bad_rows)
    with pytest.raises(ValueError, match="indptr"):
        ops.rank_rows_f32(t, 5, row_users=[0, 1], exclude=(dev[0][:-1], dev[1]))
    with pytest.raises(ValueError, match="row_users"):
        ops.rank_rows_f32(t, 5, exclude=dev)
    with pytest.raises(ValueError, match="row_users"):
        ops.rank_rows_f32(t, 5, row_users=[0], exclude=dev)
    with pytest.raises(ValueError, match="cap of 128"):
        ops.rank_rows_f32(t, 129)
    with pytest.raises(ValueError, match="topk=0"):
        ops.rank_rows_f32(t, 0)
    with pytest.raises(TypeError):
        ops.rank_rows_f32(t.double(), 5)
    with pytest.raises(ValueError, match="contiguous"):
        ops.rank_rows_f32(torch.zeros(I, 2, device="cuda").t(), 5)
    with pytest.raises(RuntimeError, match="device memory"):
        ops.rank_rows_f32(torch.zeros(2, I), 5)
    assert ops.rank_rows_f32(t[:0], 5).shape == (0, 5)
    assert ops.rank_rows_f32(t[:, :7], 50).shape == (2, 7)             # topk truncates to I like full_rank_users
    # an empty exclusion list is not an error
    empty, _ = _csr([np.zeros(0, np.int32)] * U)
    assert torch.equal(ops.rank_rows_f32(t, 5, row_users=[3, 4], exclude=empty), ops.rank_rows_f32(t, 5))
