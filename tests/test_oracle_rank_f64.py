"""tests/rank_f64_oracle.py against hand-written cases and the lists the REAL reference's models ranked (the goldens of
EASE, ItemKNN / UserKNN, PureSVD and SLiM), and the argument checks of the four daisy_*_full_rank_users entries
(DESIGN.md §25).  CPU only."""
import ctypes
import os
import re

import numpy as np
import pytest

import rank_f64_oracle as RO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAN, INF = float("nan"), float("inf")


# ---- the oracle on hand-written cases ----------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_id_and_zeros_are_one_value():
    s = np.array([[1.0, 3.0, 3.0, -0.0, 0.0, 3.0, 2.0]])
    ids, sc = RO.rank_lists(s, 7)
    assert ids.tolist() == [[1, 2, 5, 6, 0, 3, 4]]
    assert sc.tolist() == [[3.0, 3.0, 3.0, 2.0, 1.0, 0.0, 0.0]] and not np.signbit(sc).any()
    ids, _ = RO.rank_lists(np.array([[-0.0, 0.0, -0.0]]), 2)
    assert ids.tolist() == [[0, 1]]


def test_nan_is_never_selected_and_infinities_are_ordered():
    s = np.array([[NAN, 1.0, INF, -INF, NAN, 2.0]])
    ids, sc = RO.rank_lists(s, 6)
    assert ids.tolist() == [[2, 5, 1, 3, -1, -1]]
    assert sc[0, :4].tolist() == [INF, 2.0, 1.0, -INF] and np.isneginf(sc[0, 4:]).all()
    ids, sc = RO.rank_lists(np.full((1, 4), NAN), 3)
    assert ids.tolist() == [[-1, -1, -1]] and np.isneginf(sc).all()


def test_exclusion_forms_all_excluded_and_topk_above_the_item_count():
    s = np.array([[5.0, 4.0, 3.0, 2.0], [5.0, 4.0, 3.0, 2.0], [1.0, 1.0, 1.0, 1.0]])
    users = [2, 0, 1]
    as_dict = {2: {0, 2}, 0: {0, 1, 2, 3}}
    ids, sc = RO.rank_lists(s, 6, users=users, exclude=as_dict)
    assert ids.tolist() == [[1, 3, -1, -1, -1, -1], [-1] * 6, [0, 1, 2, 3, -1, -1]]
    assert sc[0, :2].tolist() == [4.0, 2.0] and np.isneginf(sc[1]).all()
    csr = RO.user_csr(as_dict, 3)
    assert csr[0].tolist() == [0, 4, 4, 6] and csr[1].tolist() == [0, 1, 2, 3, 0, 2]
    ids2, sc2 = RO.rank_lists(s, 6, users=users, exclude=csr)
    assert np.array_equal(ids, ids2) and np.array_equal(sc, sc2)
    # duplicates and an entry past the last item change nothing
    dup = (np.array([0, 0, 0, 4]), np.array([0, 0, 2, 9], np.int32))
    assert RO.rank_lists(s[:1], 6, users=[2], exclude=dup)[0].tolist() == [[1, 3, -1, -1, -1, -1]]
    # float32 rows keep their dtype
    ids, sc = RO.rank_lists(s.astype(np.float32), 2)
    assert sc.dtype == np.float32 and ids.tolist() == [[0, 1], [0, 1], [0, 1]]


# ---- the oracle against the reference's lists ----------------------------------------------------------------------------------
def _lists_over_candidates(scores, cands, topk):
    """the oracle over the candidates' POSITIONS, mapped to their ids: the reference ranks candidates, and a tie falls to
    the lower position there as it falls to the lower id in a full ranking"""
    pos, _ = RO.rank_lists(scores, topk)
    assert (pos >= 0).all()
    return np.take_along_axis(cands, pos, 1)


@pytest.mark.parametrize("name,score_key", [("kat_ease.npz", "scores_ref"), ("kat_knn.npz", "scores_ref"),
                                            ("kat_puresvd.npz", "scores_ref"), ("kat_slim.npz", "A_ref")])
def test_oracle_reproduces_the_lists_of_the_goldens(name, score_key):
    k = np.load(os.path.join(HERE, "golden", name))
    checked = 0
    for tag in k["tags"].tolist():
        keys = [f"{tag}_{x}" for x in (score_key, "cands", "rank_ref")]
        if not all(x in k.files for x in keys):
            continue                                    # (kat_knn's similarity-only fixtures store no lists)
        scores, cands, ref = (k[x] for x in keys)
        assert scores.shape == cands.shape and scores.dtype == np.float64 and ref.shape[0] == cands.shape[0]
        got = _lists_over_candidates(scores, cands, ref.shape[1])
        if name == "kat_slim.npz":
            # the reference's unstable argsort leaves exact ties open (tests/test_oracle_slim.py): rows whose candidate
            # scores are all distinct are decided by the scores alone
            rows = np.array([len(set(r.tolist())) == r.size for r in scores])
            assert rows.sum() >= scores.shape[0] // 2, (tag, int(rows.sum()))
        elif name == "kat_puresvd.npz":
            # a list is decided by the stored scores where its first topk + 1 of them lie further apart than the
            # fixture's own bound (tests/test_oracle_puresvd.py: 1e4 x 100 x oracle_dev); the rank-deficient fixture
            # holds scores that differ in the last bits only
            top = -np.sort(-scores, 1)[:, :ref.shape[1] + 1]
            rows = (top[:, :-1] - top[:, 1:]).min(1) >= 1e6 * float(k[f"{tag}_oracle_dev"])
        else:
            rows = np.ones(scores.shape[0], bool)
        assert np.array_equal(got[rows], ref[rows]), (name, tag)
        checked += int(rows.sum())
    assert checked >= 100, (name, checked)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
ENTRIES = ("ease", "slim", "knn", "psvd")
C_TYPES = {"const int64_t *": "p", "const int32_t *": "p", "const float *": "p", "const double *": "p", "int64_t *": "p",
           "double *": "p", "float *": "p", "daisy_stream_t": "p", "int64_t": "i64", "int32_t": "i32"}


def _header_signature(name):
    src = open(os.path.join(ROOT, "include", "daisyrec_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in the header"
    out = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        ctype = arg[:arg.rindex(" ") + 1].strip() if "*" not in arg else arg[:arg.rindex("*") + 1]
        out.append(C_TYPES[ctype.strip()])
    return out


def test_ctypes_signatures_are_the_headers():
    from daisyrec_amd import _native as N
    names = {"p": ctypes.c_void_p, "i64": ctypes.c_int64, "i32": ctypes.c_int32}
    for e in ENTRIES:
        res, args = N.SIGNATURES[f"daisy_{e}_full_rank_users"]
        assert res is ctypes.c_int
        assert args == [names[a] for a in _header_signature(f"daisy_{e}_full_rank_users")], e
    assert N.SIGNATURES["daisy_rank_f64_users_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64,
                                                                                    ctypes.c_int32])
    assert N.ABI_VERSION == 8


def _call(N, entry, d, **over):
    a = dict(m0=d, m1=d, m2=d, m3=d, m4=d, m5=d, U=50, I=1000, inner=1000, k=16, users=d, n=4, indptr=None, items=None,
             topk=10, ids=d, scores=None, path=0)
    a.update(over)
    tail = (a["users"], a["n"], a["indptr"], a["items"], a["topk"], a["ids"], a["scores"])
    if entry == "ease":
        return N.lib.daisy_ease_full_rank_users(a["m0"], a["m1"], a["m2"], a["m3"], a["U"], a["I"], *tail, None)
    if entry == "slim":
        return N.lib.daisy_slim_full_rank_users(a["m0"], a["m1"], a["m2"], a["U"], a["I"], a["m3"], a["m4"], a["m5"], *tail,
                                                a["path"], None)
    if entry == "knn":
        return N.lib.daisy_knn_full_rank_users(a["m0"], a["m1"], a["m2"], a["U"], a["inner"], a["m3"], a["m4"], a["m5"],
                                               a["I"], *tail, a["path"], None)
    return N.lib.daisy_psvd_full_rank_users(a["m0"], a["m1"], a["U"], a["I"], a["k"], *tail, None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_do_not_need_a_gpu(entry):
    """every check precedes the first HIP call (the pointers are dummies nobody reads)"""
    from daisyrec_amd import _native as N
    buf = ctypes.create_string_buffer(256)
    d = ctypes.addressof(buf)
    cases = [(dict(m0=None), "NULL"), (dict(m1=None), "NULL"), (dict(users=None), "NULL"), (dict(ids=None), "NULL"),
             (dict(topk=0), "topk=0"), (dict(topk=-3), "topk=-3"), (dict(topk=129), "cap of 128"),
             (dict(indptr=d), "excl_indptr"), (dict(items=d), "excl_indptr"), (dict(n=-1), "n=-1"),
             (dict(I=0), "item_num=0"), (dict(U=0), "user_num=0")]
    if entry != "psvd":
        cases += [(dict(m2=None), "NULL"), (dict(m3=None), "NULL")]
    if entry in ("slim", "knn"):
        cases += [(dict(m4=None), "NULL"), (dict(m5=None), "NULL"), (dict(path=3), "path=3"), (dict(path=-1), "path=-1"),
                  (dict(path=1, I=40000, inner=40000), "LDS path")]
    if entry == "knn":
        cases += [(dict(inner=0), "inner=0")]
    if entry == "psvd":
        cases += [(dict(k=0), "k=0"), (dict(k=100000), "k=100000")]
    for over, text in cases:
        rc = _call(N, entry, d, **over)
        assert rc == N.DAISY_ERR_ARG, (over, rc)
        msg = N.last_error()
        assert msg.startswith(f"{entry}_full_rank_users:") and text in msg, (over, msg)
    with pytest.raises(ValueError, match="cap of 128"):
        N.check(_call(N, entry, d, topk=129))
    # no user: DAISY_OK without a launch (and without a device), the other arguments still checked first
    assert _call(N, entry, d, n=0) == N.DAISY_OK
    assert _call(N, entry, d, n=0, users=None, ids=None) == N.DAISY_OK
    assert _call(N, entry, d, n=0, topk=129) == N.DAISY_ERR_ARG
    # topk above the item count is allowed: the tail of such a list is -1
    assert _call(N, entry, d, n=0, topk=128, I=5, inner=5) == N.DAISY_OK


def test_no_workspace_at_any_shape():
    from daisyrec_amd import _native as N
    ws = N.lib.daisy_rank_f64_users_workspace_bytes
    assert ws(138493, 26744, 50) == 0 and ws(1 << 30, 1 << 30, 128) == 0 and ws(0, 0, 0) == 0
