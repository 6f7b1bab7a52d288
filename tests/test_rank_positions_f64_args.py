"""The argument checks of daisy_{ease,slim,knn,psvd}_full_rank_positions and daisy_rank_rows_positions_f32
through ctypes: every check precedes the first HIP call, so the pointers are dummies nobody reads.  CPU only.  Fails
without the feature (the library has no such symbols)."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def N():
    from daisyrec_amd import _native
    return _native


@pytest.fixture(scope="module")
def d():
    buf = ctypes.create_string_buffer(256)
    yield ctypes.addressof(buf)
    del buf


# the arguments of every entry in header order; `model` names the operand pointers that must not be NULL
def _ease(N, d, **o):
    a = dict(row_ptr=d, col=d, val=d, W=d, U=50, I=1000, users=d, n=4, indptr=None, items=None, tp=d, ti=d, op=d, T=40, pos=d,
             scores=None, elig=None)
    a.update(o)
    return N.lib.daisy_ease_full_rank_positions(a["row_ptr"], a["col"], a["val"], a["W"], a["U"], a["I"], a["users"], a["n"],
                                                a["indptr"], a["items"], a["tp"], a["ti"], a["op"], a["T"], a["pos"], a["scores"],
                                                a["elig"], None)


def _slim(N, d, **o):
    a = dict(row_ptr=d, col=d, val=d, U=50, I=1000, w_ptr=d, w_row=d, w_val=d, users=d, n=4, indptr=None, items=None, tp=d, ti=d,
             op=d, T=40, pos=d, scores=None, elig=None, path=0)
    a.update(o)
    return N.lib.daisy_slim_full_rank_positions(a["row_ptr"], a["col"], a["val"], a["U"], a["I"], a["w_ptr"], a["w_row"], a["w_val"],
                                                a["users"], a["n"], a["indptr"], a["items"], a["tp"], a["ti"], a["op"], a["T"],
                                                a["pos"], a["scores"], a["elig"], a["path"], None)


def _knn(N, d, **o):
    a = dict(l_ptr=d, l_col=d, l_val=d, U=50, inner=60, r_ptr=d, r_row=d, r_val=d, I=1000, users=d, n=4, indptr=None, items=None,
             tp=d, ti=d, op=d, T=40, pos=d, scores=None, elig=None, path=0)
    a.update(o)
    return N.lib.daisy_knn_full_rank_positions(a["l_ptr"], a["l_col"], a["l_val"], a["U"], a["inner"], a["r_ptr"], a["r_row"],
                                               a["r_val"], a["I"], a["users"], a["n"], a["indptr"], a["items"], a["tp"], a["ti"],
                                               a["op"], a["T"], a["pos"], a["scores"], a["elig"], a["path"], None)


def _psvd(N, d, **o):
    a = dict(uv=d, iv=d, U=50, I=1000, k=8, users=d, n=4, indptr=None, items=None, tp=d, ti=d, op=d, T=40, pos=d, scores=None,
             elig=None)
    a.update(o)
    return N.lib.daisy_psvd_full_rank_positions(a["uv"], a["iv"], a["U"], a["I"], a["k"], a["users"], a["n"], a["indptr"],
                                                a["items"], a["tp"], a["ti"], a["op"], a["T"], a["pos"], a["scores"], a["elig"], None)


def _rows(N, d, **o):
    a = dict(scores_in=d, n=4, I=1000, pitch=1000, users=d, indptr=None, items=None, tp=d, ti=d, op=d, T=40, pos=d, scores=None,
             elig=None)
    a.update(o)
    return N.lib.daisy_rank_rows_positions_f32(a["scores_in"], a["n"], a["I"], a["pitch"], a["users"], a["indptr"], a["items"],
                                               a["tp"], a["ti"], a["op"], a["T"], a["pos"], a["scores"], a["elig"], None)


ENTRIES = {"ease_full_rank_positions": (_ease, ("row_ptr", "col", "val", "W")),
           "slim_full_rank_positions": (_slim, ("row_ptr", "col", "val", "w_ptr", "w_row", "w_val")),
           "knn_full_rank_positions": (_knn, ("l_ptr", "l_col", "l_val", "r_ptr", "r_row", "r_val")),
           "psvd_full_rank_positions": (_psvd, ("uv", "iv")),
           "rank_rows_positions_f32": (_rows, ("scores_in",))}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_every_argument_error(N, d, name):
    call, model = ENTRIES[name]
    cases = [({p: None}, "NULL") for p in model + ("users", "tp", "op", "ti", "pos")]
    cases += [(dict(indptr=d), "together"), (dict(items=d), "together"),
              (dict(I=0), "item_num=0"), (dict(I=-3), "item_num=-3"), (dict(I=1 << 31), "item_num=2147483648"),
              (dict(n=-1), "=-1"), (dict(T=-1), "n_targets=-1")]
    if name == "rank_rows_positions_f32":
        cases += [(dict(pitch=999), "pitch=999"), (dict(n=(1 << 31)), "row count")]
    else:
        cases += [(dict(U=0), "user_num=0"), (dict(n=(1 << 31)), "request count")]
    if name in ("slim_full_rank_positions", "knn_full_rank_positions"):
        cases += [(dict(path=3), "path=3"), (dict(path=-1), "path=-1")]
        cases += [(dict(path=1, I=40000), "LDS path")] if name == "slim_full_rank_positions" else \
            [(dict(inner=0), "inner=0"), (dict(path=1, inner=40000), "LDS path")]
    if name == "psvd_full_rank_positions":
        cases += [(dict(k=0), "k=0"), (dict(k=100000), "k=100000")]
    for over, text in cases:
        rc = call(N, d, **over)
        assert rc == N.DAISY_ERR_ARG, (name, over, rc)
        msg = N.last_error()
        assert msg.startswith(name + ":") and text in msg, (name, over, msg)


@pytest.mark.parametrize("name", list(ENTRIES))
def test_nothing_to_do_is_ok_without_a_launch(N, d, name):
    call, _ = ENTRIES[name]
    assert call(N, d, n=0) == N.DAISY_OK
    assert call(N, d, n=0, users=None, tp=None, ti=None, op=None, pos=None, T=0) == N.DAISY_OK
    # no targets and no eligible count asked for: nothing to write, whatever n
    assert call(N, d, T=0, ti=None, pos=None) == N.DAISY_OK
    # but the other checks still come first
    assert call(N, d, n=0, I=0) == N.DAISY_ERR_ARG
    assert call(N, d, n=0, indptr=d) == N.DAISY_ERR_ARG
