"""EASE on the host: the reference's UNMODIFIED run_examples/test.py with --algo_name ease reaches `fit` of daisyrec_amd's
EASE (dropin.install()), which refuses to run without a device (no CPU fallback); constructor and argument errors; the
argument checks of the daisy_ease_* entry points (before any HIP call)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_oracle_ease import ease_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("DAISY_REFERENCE", "/root/reference")
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "daisy")), reason="reference checkout not present")
host_only = pytest.mark.skipif(torch.cuda.is_available(), reason="host-only check (with a device the run would train)")


@needs_ref
@host_only
def test_reference_driver_reaches_the_hip_ease(tmp_path):
    d = tmp_path / "daisy_checkout"                        # writable cwd: the driver writes ./log ./res
    d.mkdir()
    for name in ("daisy", "run_examples", "data"):
        os.symlink(os.path.join(REF, name), d / name)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_daisy_example.py"), "--daisy", str(d), "--",
                        "--algo_name", "ease"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "no HIP device visible" in r.stderr, r.stderr[-2000:]
    assert "model.fit(train_set)" in r.stderr, r.stderr[-2000:]
    assert os.path.join("daisyrec_amd", "model", "EASERecommender.py") in r.stderr, r.stderr[-2000:]


def test_dropin_rebinds_the_reference_name():
    if not os.path.isdir(os.path.join(REF, "daisy")):
        pytest.skip("reference checkout not present")
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import daisyrec_amd.dropin as d; d.install()\n"
            "import daisy.model.EASERecommender as m; from daisyrec_amd.model import EASE\n"
            "assert m.EASE is EASE\n") % (os.path.join(ROOT, "tests", "golden", "_shims"), REF, ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def _frame(u, i, r, names=("user", "item", "rating")):
    import pandas as pd
    return pd.DataFrame(dict(zip(names, (u, i, r))))


def test_surface_errors_without_a_device():
    from daisyrec_amd.model import EASE
    m = EASE(ease_config())
    assert (m.reg_weight, m.topk, m.user_num, m.item_num) == (200.0, 10, 3, 4)
    assert (m.uid_name, m.iid_name, m.inter_name) == ("user", "item", "rating")
    assert m.item_similarity is None and m.interaction_matrix is None and m.fit_info is None
    for over, msg in ((dict(reg=0), "reg"), (dict(reg=0.0), "reg"), (dict(reg=-1), "reg"), (dict(reg=float("nan")), "reg"),
                      (dict(reg=float("inf")), "reg"), (dict(topk=0), "topk"), (dict(item_num=0), "item_num"),
                      (dict(user_num=0), "user_num")):
        with pytest.raises(ValueError, match=msg):
            EASE(ease_config(**over))
    for frame, msg in ((_frame([0, 3], [0, 1], [1., 1.]), "user id 3"), (_frame([0, 1], [0, 4], [1., 1.]), "item id 4"),
                       (_frame([0, -1], [0, 1], [1., 1.]), "user id -1"), (_frame([0, 1], [0, 1], [1., np.nan]), "finite"),
                       (_frame([0, 1], [0, 1], [1., np.inf]), "finite"), (_frame([0, 0.5], [0, 1], [1., 1.]), "non-integer")):
        with pytest.raises(ValueError, match=msg):
            m.fit(frame)
    with pytest.raises(KeyError):
        m.fit(_frame([0], [0], [1.]).rename(columns={"rating": "label"}))
    # the configured column names are the ones read (the reference's config['UID_NAME'] ...)
    named = EASE(ease_config(UID_NAME="uid", IID_NAME="iid", INTER_NAME="click"))
    with pytest.raises(KeyError):
        named.fit(_frame([0], [0], [1.]))
    with pytest.raises(ValueError, match="column 'click'"):
        named.fit(_frame([0], [0], [np.nan], names=("uid", "iid", "click")))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device visible"):
            m.fit(_frame([0, 1], [0, 1], [1., 1.]))
        with pytest.raises(RuntimeError, match="no HIP device visible"):
            named.fit(_frame([0], [0], [1.], names=("uid", "iid", "click")))
        with pytest.raises(RuntimeError, match="no HIP device visible"):
            m.full_rank(0)


def test_ease_abi_argument_errors():
    from daisyrec_amd import _native as N
    L = N.lib
    buf = ctypes.create_string_buffer(256)
    d = ctypes.addressof(buf)                              # a dummy pointer nobody reads
    d2 = d + 64
    # sizes: ceil(n / 64) blocks of 64 x 64 doubles plus n doubles; the peak of a fit is TWO n^2 fp64 buffers plus that
    assert L.daisy_ease_workspace_bytes(0) == 0 and L.daisy_ease_workspace_bytes(-3) == 0
    assert L.daisy_ease_workspace_bytes(1 << 40) == 0 and L.daisy_ease_fit_bytes(0) == 0
    assert 32768 + 8 <= L.daisy_ease_workspace_bytes(1) <= 32768 + 256
    assert 3 * 32768 + 130 * 8 <= L.daisy_ease_workspace_bytes(130) <= 3 * 32768 + 130 * 8 + 512
    big = 46341                                            # n^2 passes 2^31: the byte counts are 64-bit
    ws = L.daisy_ease_workspace_bytes(big)
    assert 2 * big * big * 8 + ws <= L.daisy_ease_fit_bytes(big) <= 2 * big * big * 8 + ws + 512
    assert L.daisy_ease_fit_bytes(big) < 3 * big * big * 8                      # at most three such buffers: it is two
    assert L.daisy_ease_fits(1682, 1 << 30) == N.DAISY_OK
    assert L.daisy_ease_fits(1682, L.daisy_ease_fit_bytes(1682)) == N.DAISY_OK
    assert L.daisy_ease_fits(1682, L.daisy_ease_fit_bytes(1682) - 1) == N.DAISY_ERR_ARG
    assert N.last_error().startswith("ease_fits:") and "does not fit" in N.last_error() and "two fp64" in N.last_error()
    assert L.daisy_ease_fits(40000, 1 << 30) == N.DAISY_ERR_ARG and "1073741824 bytes offered" in N.last_error()
    assert L.daisy_ease_fits(0, 1 << 30) == N.DAISY_ERR_ARG and "item_num" in N.last_error()
    assert L.daisy_ease_fits(1 << 40, (1 << 64) - 1) == N.DAISY_ERR_ARG and "item_num" in N.last_error()

    def expect(rc, name, msg, what):
        assert rc == N.DAISY_ERR_ARG, what
        assert N.last_error().startswith(name + ":") and msg in N.last_error(), (what, N.last_error())

    W = 1 << 20
    for kw, msg in ((dict(G=None), "NULL"), (dict(A=None), "NULL"), (dict(n=0), "item_num"), (dict(n=1 << 40), "item_num"),
                    (dict(reg=float("nan")), "reg")):
        a = dict(G=d, n=40, reg=200.0, A=d)
        a.update(kw)
        expect(L.daisy_ease_system(a["G"], a["n"], a["reg"], a["A"], None), "ease_system", msg, kw)
    for kw, msg in ((dict(A=None), "NULL"), (dict(info=None), "NULL"), (dict(ws=None), "NULL"), (dict(n=0), "n="),
                    (dict(n=-5), "n="), (dict(n=1 << 40), "n="), (dict(wsb=64), "workspace"), (dict(n=130, wsb=3 * 32768), "workspace")):
        a = dict(A=d, n=40, info=d, ws=d, wsb=W)
        a.update(kw)
        expect(L.daisy_ease_potrf(a["A"], a["n"], a["info"], a["ws"], a["wsb"], None), "ease_potrf", msg, kw)
    for kw, msg in ((dict(L=None), "NULL"), (dict(T=None), "NULL"), (dict(P=None), "NULL"), (dict(ws=None), "NULL"),
                    (dict(n=0), "n="), (dict(T=d), "T must be"), (dict(T=d2, P=d2), "T must be"), (dict(wsb=64), "workspace")):
        a = dict(L=d, n=40, T=d2, P=d, ws=d, wsb=W)
        a.update(kw)
        expect(L.daisy_ease_potri(a["L"], a["n"], a["T"], a["P"], a["ws"], a["wsb"], None), "ease_potri", msg, kw)
    for kw, msg in ((dict(P=None), "NULL"), (dict(B=None), "NULL"), (dict(ws=None), "NULL"), (dict(n=0), "n="),
                    (dict(wsb=64), "workspace")):
        a = dict(P=d, n=40, B=d, ws=d, wsb=W)
        a.update(kw)
        expect(L.daisy_ease_weights(a["P"], a["n"], a["B"], a["ws"], a["wsb"], None), "ease_weights", msg, kw)

    def rank(rp=d, col=d, val=d, Wm=d, U=10, I=40, users=d, B=4, items=d, Cn=3, topk=2, scores=d, ids=d):
        return L.daisy_ease_rank(rp, col, val, Wm, U, I, users, B, items, Cn, topk, scores, ids, None)
    for kw, msg in ((dict(rp=None), "NULL"), (dict(col=None), "NULL"), (dict(val=None), "NULL"), (dict(Wm=None), "NULL"),
                    (dict(scores=None), "NULL"), (dict(U=0), "user_num"), (dict(I=0), "item_num"), (dict(users=None), "users"),
                    (dict(B=-1), "B="), (dict(Cn=0), "candidates"), (dict(items=None, Cn=3), "candidates"),
                    (dict(topk=0), "topk"), (dict(topk=4), "topk")):
        expect(rank(**kw), "ease_rank", msg, kw)
    assert rank(B=0) == N.DAISY_OK                          # nothing to do: no launch
