"""tests/full_rank_oracle.py against the lists the REAL reference's MF.full_rank / FM.full_rank produced
(tests/golden/make_golden_full_rank.py), and the argument checks of daisy_full_rank_users.  CPU only."""
import ctypes
import os

import numpy as np
import pytest

import full_rank_oracle as FO

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(HERE, "golden", "kat_full_rank.npz"))


def test_exact_oracle_equals_the_reference_lists(kat):
    P, Q, topk = kat["P"], kat["Q"], int(kat["topk"])
    users = np.arange(P.shape[0])
    ids, scores = FO.full_rank_exact(P, Q, users, topk)
    assert np.array_equal(ids, kat["full_mf"])
    assert np.array_equal(scores, (P.astype(np.int64) @ Q.astype(np.int64).T)[users[:, None], ids].astype(np.float32))
    ids_fm, _ = FO.full_rank_exact(P, Q, users, topk, biases=(kat["bu"], kat["bi"], kat["b0"]))
    assert np.array_equal(ids_fm, kat["full_fm"])
    assert not np.array_equal(ids_fm, ids)                  # the biases matter on this fixture


def test_exact_oracle_exclusion_fill_and_ties(kat):
    P, Q = kat["P"], kat["Q"]
    I = Q.shape[0]
    full = kat["full_mf"]
    excl = {0: set(full[0, :3].tolist()), 1: set(range(I)), 2: set(range(I - 4))}
    ids, scores = FO.full_rank_exact(P, Q, np.array([0, 1, 2, 0]), 10, exclude=excl)
    all0, _ = FO.full_rank_exact(P, Q, np.array([0]), 13)
    assert np.array_equal(ids[0], all0[0, 3:]) and np.array_equal(ids[3], ids[0])
    assert np.all(ids[1] == -1) and np.all(np.isneginf(scores[1]))
    assert set(ids[2, :4].tolist()) == set(range(I - 4, I)) and np.all(ids[2, 4:] == -1)
    Z = np.zeros_like(Q)
    ids, scores = FO.full_rank_exact(P, Z, np.array([5]), 4, exclude={5: {0, 2}})
    assert ids.tolist() == [[1, 3, 4, 5]] and np.all(scores == 0)
    # the CSR form of the same exclusion
    indptr = np.zeros(P.shape[0] + 1, np.int64)
    indptr[6:] = 2
    ids2, _ = FO.full_rank_exact(P, Z, np.array([5]), 4, exclude=(indptr, np.array([0, 2], np.int32)))
    assert np.array_equal(ids2, ids)


def test_toleranced_check_accepts_fp32_and_rejects_a_wrong_list():
    rng = np.random.default_rng(2022)
    P = rng.normal(0, 0.1, (20, 64)).astype(np.float32)
    Q = rng.normal(0, 0.1, (300, 64)).astype(np.float32)
    users = np.arange(20)
    s32 = (P @ Q.T).astype(np.float32)
    ids, scores = FO.rank_lists(s32, FO.exclusion_sets(None, users), 50)
    FO.check_toleranced(P, Q, users, 50, ids, scores)
    bad = ids.copy()
    worst = np.argsort(s32[0])[0]
    bad[0, -1] = worst
    bad_scores = scores.copy()
    bad_scores[0, -1] = s32[0, worst]
    with pytest.raises(AssertionError):
        FO.check_toleranced(P, Q, users, 50, bad, bad_scores)


def _call(N, buf, **over):
    d = ctypes.addressof(buf)
    a = dict(P=d, Q=d, bu=None, bi=None, b0=None, d=16, I=1000, users=d, n=4, indptr=None, items=None, topk=10, slices=0,
             ids=d, scores=None, ws=d, ws_bytes=1 << 40)
    a.update(over)
    return N.lib.daisy_full_rank_users(a["P"], a["Q"], a["bu"], a["bi"], a["b0"], a["d"], a["I"], a["users"], a["n"],
                                       a["indptr"], a["items"], a["topk"], a["slices"], a["ids"], a["scores"], a["ws"],
                                       a["ws_bytes"], None)


def test_argument_errors_do_not_need_a_gpu():
    """every check precedes the first HIP call (the pointers are dummies nobody reads)"""
    from daisyrec_amd import _native as N
    buf = ctypes.create_string_buffer(256)
    d = ctypes.addressof(buf)
    cases = [(dict(P=None), "NULL"), (dict(Q=None), "NULL"), (dict(topk=0), "topk=0"),
             (dict(topk=129), "cap of 128"), (dict(d=100000), "d=100000"), (dict(d=0), "d=0"),
             (dict(indptr=d), "excl_indptr"), (dict(items=d), "excl_indptr"), (dict(bu=d), "u_bias"),
             (dict(bu=d, bi=d), "u_bias"), (dict(n=0), "n=0"), (dict(I=0), "item_num=0"), (dict(I=1 << 31), "item_num="),
             (dict(topk=11, I=10), "topk=11"), (dict(slices=-1), "item_slices"), (dict(ws_bytes=8), "workspace"),
             (dict(users=None), "NULL"), (dict(ids=None), "NULL"), (dict(ws=None), "NULL")]
    for over, text in cases:
        rc = _call(N, buf, **over)
        assert rc == N.DAISY_ERR_ARG, (over, rc)
        msg = N.last_error()
        assert msg.startswith("full_rank_users:") and text in msg, (over, msg)
    with pytest.raises(ValueError, match="cap of 128"):
        N.check(_call(N, buf, topk=129))


def test_workspace_is_far_below_a_score_matrix():
    from daisyrec_amd import _native as N
    ws = N.lib.daisy_full_rank_users_workspace_bytes
    n, I = 1 << 20, 1 << 17
    assert 0 < ws(n, I, 50, 0) < n * I * 4 // 1000
    assert ws(0, 10, 5, 0) == 0
    assert ws(10, 10, 129, 0) == 0 and ws(10, 0, 5, 0) == 0
    # one partial list of topk sort words per user and item slice; slices are clamped to the 128-item tiles
    up = lambda x: (x + 255) // 256 * 256         # noqa: E731
    assert ws(100, 1000, 10, 1) == up(100 * 10 * 8)
    assert ws(100, 1000, 10, 1000) == ws(100, 1000, 10, 8) == up(100 * 8 * 10 * 8)
    assert ws(100, 1000, 10, 3) == up(100 * 3 * 10 * 8)
