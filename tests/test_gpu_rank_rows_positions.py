"""ops.rank_rows_positions_f32 (csrc/rank_rows_positions.hip): positions, score bits and eligible counts
against a numpy sort by §24's sort word, and against the lists of ops.rank_rows_f32 with the same arguments, for every size
around the kernel's step, both load paths, every kind of row content, exclusion edge and target-row length.  Every test
here fails without the feature (AttributeError)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
U = 9                           # rows of the exclusion and target CSRs
TC = 512                        # kRcTc (csrc/rank_count.h): targets a workgroup ranks per pass over the row
FEW = 16                        # kRcFew: blocks of fewer ranked targets count bucket by bucket
STEP = 1024                     # kRrpStep: items a workgroup takes per step
SIZES = (1, 3, STEP - 1, STEP, STEP + 1, 2 * STEP + 37)
NAN, INF = np.float32("nan"), np.float32("inf")


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _csr(rows):
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    items = np.concatenate([np.asarray(r, np.int32) for r in rows]) if indptr[-1] else np.zeros(0, np.int32)
    return indptr, items


def words(row):
    """§24's sort word of every item of a float32 row (csrc/rank_key_f32.h): (order-preserving key << 32) | (0xFFFFFFFF - id)"""
    v = (np.asarray(row, np.float32) + np.float32(0.0))         # -0.0 -> +0.0
    b = v.view(np.uint32).astype(np.uint64)
    key = np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000)
    key = np.where(np.isnan(v), 0xFFFFFFFF, key).astype(np.uint64)
    return (key << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(v.size, dtype=np.uint64))


def oracle(s, row_users, targets, exclude):
    """(out_indptr, pos, scores, eligible) of score rows s [m, I] by sorting the words"""
    m, I = s.shape
    t_indptr, t_items = targets
    rows = [t_items[t_indptr[u]:t_indptr[u + 1]].tolist() for u in row_users]
    out_indptr = np.zeros(m + 1, np.int64)
    out_indptr[1:] = np.cumsum([len(r) for r in rows])
    pos = np.full(out_indptr[-1], -1, np.int32)
    sc = np.full(out_indptr[-1], -np.inf, np.float32)
    eligible = np.zeros(m, np.int32)
    for r, u in enumerate(row_users):
        ok = np.ones(I, bool)
        if exclude is not None:
            e = exclude[1][exclude[0][u]:exclude[0][u + 1]].astype(np.int64)
            ok[e[(e >= 0) & (e < I)]] = False
        w = words(s[r])
        order = np.sort(w[ok])[::-1]                            # largest word first
        eligible[r] = order.size
        for j, t in enumerate(rows[r]):
            if 0 <= t < I and ok[t]:
                pos[out_indptr[r] + j] = int((order > w[t]).sum())
                sc[out_indptr[r] + j] = s[r, t]
    return out_indptr, pos, sc, eligible


def _content(rng, m, I):
    """integer-valued scores with heavy ties; row 1 all equal; a NaN, both zeros and both infinities where there is room"""
    s = rng.integers(-3, 4, size=(m, I)).astype(np.float32)
    if m > 1:
        s[1] = 2.0
    if I >= 3:
        s[0, [0, 1, 2]] = (-0.0, 0.0, NAN)
    if I > STEP:
        s[0, [STEP - 1, STEP, I - 1]] = (INF, -INF, NAN)
        s[m - 1, [5, STEP - 2, I - 2]] = (-0.0, INF, -INF)
    return s


def _exclusion(rng, I):
    """entries at 0, at the step edges and at I - 1, repeated entries, an empty row, a full row, entries past the end"""
    edge = sorted({0, min(STEP - 1, I - 1), min(STEP, I - 1), min(2 * STEP - 1, I - 1), I - 1})
    rows = [edge, [], list(range(I)), sorted(edge + edge), [0], [I - 1, I, I + 5, 2 ** 31 - 1]]
    rows += [np.sort(rng.choice(I, max(1, I // 5), replace=False)).tolist() for _ in range(U - len(rows))]
    return _csr(rows)


def _targets(rng, I):
    """rows of 0, 1, Tc - 1, Tc, Tc + 1 and I targets, as far as I allows, then rows around FEW; ascending, no repeats"""
    lens = [0, 1, TC - 1, TC, TC + 1, I, FEW - 1, FEW, FEW + 1]
    assert len(lens) == U
    return _csr([np.sort(rng.choice(I, min(k, I), replace=False)).tolist() for k in lens])


def _layouts(s):
    """the same values as a contiguous matrix, as a column slice of a wider one at an odd offset (element loads) and as a
    16-byte aligned slice with a pitch that is a multiple of 4 (float4 loads, whatever I is)"""
    m, I = s.shape
    odd = torch.zeros(m, I + 6 + (I % 2 == 0), dtype=torch.float32, device="cuda")
    odd[:, 3:3 + I] = _t(s)
    vec = torch.zeros(m, I + 8 + (-I) % 4, dtype=torch.float32, device="cuda")
    vec[:, 4:4 + I] = _t(s)
    out = {"contiguous": _t(s), "odd slice": odd[:, 3:3 + I], "aligned slice": vec[:, 4:4 + I]}
    assert out["odd slice"].stride(0) % 4 != 0 or out["odd slice"].data_ptr() % 16 != 0
    assert out["aligned slice"].stride(0) % 4 == 0 and out["aligned slice"].data_ptr() % 16 == 0
    return out


def _run(t, row_users, targets, exclude, **kw):
    from daisyrec_amd import ops
    assert (TC, STEP) == (ops.RANK_COUNT_BLOCK, ops.RANK_ROWS_STEP)
    out = ops.rank_rows_positions_f32(t, _t(np.asarray(row_users, np.int64)), tuple(_t(x) for x in targets),
                                      exclude=None if exclude is None else tuple(_t(x) for x in exclude), **kw)
    assert all(x.is_cuda for x in out) and out[0].dtype == torch.int64 and out[1].dtype == torch.int32
    return tuple(x.cpu().numpy() for x in out)


def _assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "out_indptr")
    bad = np.nonzero(got[1] != want[1])[0]
    assert bad.size == 0, (what, "positions", bad[:8], got[1][bad[:8]], want[1][bad[:8]])
    assert got[2].dtype == np.float32 and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), (what, "score bits")
    assert np.array_equal(got[3], want[3]), (what, "eligible")


@pytest.mark.parametrize("I", SIZES)
def test_against_the_sorted_words_and_the_lists(I):
    from daisyrec_amd import ops
    rng = np.random.default_rng(300 + I)
    excl, targets = _exclusion(rng, I), _targets(rng, I)
    for m in (1, 5):
        s = _content(rng, m, I)
        row_users = [5] if m == 1 else [5, 3, 7, 0, 5]          # target rows of I, Tc, FEW, 0 and I again
        layouts = _layouts(s)
        for ex in (None, excl):
            want = oracle(s, row_users, targets, ex)
            for name, t in layouts.items():
                got = _run(t, row_users, targets, ex, return_scores=True, return_eligible=True)
                _assert_same(got, want, (I, m, name, ex is not None))
                # the list call with the same arguments
                topk = min(128, I)
                ids = ops.rank_rows_f32(t, topk, row_users=_t(np.asarray(row_users, np.int64)),
                                        exclude=None if ex is None else tuple(_t(x) for x in ex)).cpu().numpy()
                for r, u in enumerate(row_users):
                    p = got[1][got[0][r]:got[0][r + 1]]
                    tg = targets[1][targets[0][u]:targets[0][u + 1]]
                    listed = (p >= 0) & (p < topk)
                    assert np.array_equal(ids[r][p[listed]], tg[listed]), (I, m, name, r)
                    assert set(ids[r].tolist()) & set(tg.tolist()) == set(tg[listed].tolist()), (I, m, name, r)
    # every target-row length and every exclusion row, one score row each
    s = _content(rng, U, I)
    users = list(range(U))
    _assert_same(_run(_t(s), users, targets, excl, return_scores=True, return_eligible=True), oracle(s, users, targets, excl),
                 (I, "all rows"))


def test_an_all_equal_row_ranks_by_id():
    I = STEP + 5
    s = np.full((1, I), -1.5, np.float32)
    targets = _csr([[0, 1, STEP - 1, STEP, I - 1]])
    excl = _csr([[0, 7, STEP, STEP]])
    _, pos, sc, el = _run(_t(s), [0], targets, excl, return_scores=True, return_eligible=True)
    assert pos.tolist() == [-1, 0, STEP - 3, -1, I - 4] and el.tolist() == [I - 3]
    assert np.isneginf(sc[[0, 3]]).all() and (sc[[1, 2, 4]] == -1.5).all()


def test_nan_first_zeros_equal_and_infinities():
    s = np.array([[1.0, -0.0, NAN, 0.0, INF, -INF, NAN, 1.0]], np.float32)
    targets = _csr([list(range(8))])
    _, pos, sc = _run(_t(s), [0], targets, None, return_scores=True)
    assert pos.tolist() == [3, 5, 0, 6, 2, 7, 1, 4]             # NaN, NaN, +inf, 1, 1, -0.0, +0.0, -inf: ties by id
    assert np.array_equal(sc.view(np.uint32), s[0].view(np.uint32))       # the stored bits: the sign of a zero, the NaN


def test_bad_targets_without_validation_and_errors():
    from daisyrec_amd import ops
    I = 300
    rng = np.random.default_rng(4)
    s = rng.integers(-3, 4, size=(2, I)).astype(np.float32)
    targets = (np.array([0, 7, 9], np.int64), np.array([I, -1, 17, 5, -2 ** 31, 5, 2 ** 31 - 1, 8, 3], np.int32))
    excl = _csr([[17, 90], [3]])
    with pytest.raises(ValueError, match="ascending"):
        _run(_t(s), [0, 1], targets, excl)
    got = _run(_t(s), [0, 1], targets, excl, return_scores=True, return_eligible=True, validate=False)
    _assert_same(got, oracle(s, [0, 1], targets, excl), "bad targets")
    assert (got[1][[0, 1, 2, 4, 6, 8]] == -1).all() and got[1][3] == got[1][5] >= 0 and got[1][7] >= 0
    with pytest.raises(IndexError):
        _run(_t(s), [0, 2], targets, excl)
    with pytest.raises(ValueError, match="row_users"):
        ops.rank_rows_positions_f32(_t(s), None, tuple(_t(x) for x in targets))
    with pytest.raises(ValueError, match="row_users"):
        _run(_t(s), [0], targets, excl)
    out = _run(torch.zeros(0, I, dtype=torch.float32, device="cuda"), [], targets, excl, return_eligible=True)
    assert out[0].tolist() == [0] and out[1].size == 0 and out[2].size == 0


def test_out_writes_into_slices():
    """a caller that walks a large request in chunks of score rows: slices of one out_indptr and one eligible, the whole
    positions and scores"""
    from daisyrec_amd import ops
    I, m = STEP + 77, 5
    rng = np.random.default_rng(9)
    s = _content(rng, m, I)
    excl, targets = _exclusion(rng, I), _targets(rng, I)
    row_users = [5, 3, 6, 0, 8]
    t, ru = _t(s), _t(np.asarray(row_users, np.int64))
    tg, ex = tuple(_t(x) for x in targets), tuple(_t(x) for x in excl)
    whole = ops.rank_rows_positions_f32(t, ru, tg, exclude=ex, return_scores=True, return_eligible=True)
    out_indptr = whole[0].clone()
    pos = torch.full_like(whole[1], -7)
    sc = torch.full_like(whole[2], 123.0)
    el = torch.full_like(whole[3], -7)
    for b0, b1 in ((0, 2), (2, 5)):
        got = ops.rank_rows_positions_f32(t[b0:b1], ru[b0:b1], tg, exclude=ex, validate=False,
                                          out=(out_indptr[b0:b1 + 1], pos, sc, el[b0:b1]))
        assert got[1] is pos and got[2] is sc
        if b1 == 2:                                             # nothing past the chunk's rows is touched
            assert (pos[int(out_indptr[2]):] == -7).all() and (el[2:] == -7).all()
    for a, b in zip(whole, (out_indptr, pos, sc, el)):
        assert np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8))
    with pytest.raises(ValueError, match="out:"):
        ops.rank_rows_positions_f32(t, ru, tg, exclude=ex, out=(out_indptr[:3], pos, sc, el))
