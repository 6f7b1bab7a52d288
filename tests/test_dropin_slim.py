"""SLiM on the host: the reference's UNMODIFIED run_examples/test.py with --algo_name slim reaches `fit` of daisyrec_amd's
SLiM (dropin.install()), which refuses to run without a device (no CPU fallback); constructor and argument errors; the
argument checks of the daisy_slim_* entry points (before any HIP call)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_oracle_slim import slim_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("DAISY_REFERENCE", "/root/reference")
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "daisy")), reason="reference checkout not present")
host_only = pytest.mark.skipif(torch.cuda.is_available(), reason="host-only check (with a device the run would train)")


@needs_ref
@host_only
def test_reference_driver_reaches_the_hip_slim(tmp_path):
    d = tmp_path / "daisy_checkout"                        # writable cwd: the driver writes ./log ./res
    d.mkdir()
    for name in ("daisy", "run_examples", "data"):
        os.symlink(os.path.join(REF, name), d / name)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_daisy_example.py"), "--daisy", str(d), "--",
                        "--algo_name", "slim"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "no HIP device visible" in r.stderr, r.stderr[-2000:]
    assert "model.fit(train_set)" in r.stderr, r.stderr[-2000:]
    assert os.path.join("daisyrec_amd", "model", "SLiMRecommender.py") in r.stderr, r.stderr[-2000:]


def test_dropin_rebinds_the_reference_name():
    if not os.path.isdir(os.path.join(REF, "daisy")):
        pytest.skip("reference checkout not present")
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import daisyrec_amd.dropin as d; d.install()\n"
            "import daisy.model.SLiMRecommender as m; from daisyrec_amd.model import SLiM\n"
            "assert m.SLiM is SLiM\n") % (os.path.join(ROOT, "tests", "golden", "_shims"), REF, ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def _frame(u, i, r):
    import pandas as pd
    return pd.DataFrame({"user": u, "item": i, "rating": r})


def test_surface_errors_without_a_device():
    from daisyrec_amd.model import SLiM
    m = SLiM(slim_config())
    assert (m.alpha, m.elastic, m.topk, m.tol, m.max_iter) == (1.0, 0.1, 50, 1e-4, 100)
    assert m.w_sparse is None and m.A_tilde is None and m.fit_info is None
    assert SLiM(slim_config(slim_tol=1e-6, slim_max_iter=7)).max_iter == 7
    for over, msg in ((dict(alpha=0.0), "alpha"), (dict(alpha=-1.0), "alpha"), (dict(elastic=1.5), "elastic"),
                      (dict(elastic=-0.1), "elastic"), (dict(topk=0), "topk"), (dict(topk=5000), "topk"),
                      (dict(item_num=0), "item_num"), (dict(slim_max_iter=0), "slim_max_iter"), (dict(slim_tol=-1.0), "slim_tol")):
        with pytest.raises(ValueError, match=msg):
            SLiM(slim_config(**over))
    for frame, msg in ((_frame([0, 3], [0, 1], [1., 1.]), "user id 3"), (_frame([0, 1], [0, 4], [1., 1.]), "item id 4"),
                       (_frame([0, -1], [0, 1], [1., 1.]), "user id -1"), (_frame([0, 1], [0, 1], [1., np.nan]), "finite")):
        with pytest.raises(ValueError, match=msg):
            m.fit(frame)
    with pytest.raises(KeyError):
        m.fit(_frame([0], [0], [1.]).rename(columns={"rating": "label"}))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device visible"):
            m.fit(_frame([0, 1], [0, 1], [1., 1.]))
        with pytest.raises(RuntimeError, match="no HIP device visible"):
            m.full_rank(0)


def test_slim_abi_argument_errors():
    from daisyrec_amd import _native as N
    L = N.lib
    buf = ctypes.create_string_buffer(256)
    d = ctypes.addressof(buf)                              # a dummy pointer nobody reads
    assert L.daisy_slim_gram_workspace_bytes(10, 0, 0) == 0
    assert L.daisy_slim_gram_workspace_bytes(10, 40, 0) >= 40 * 40 * 4 + 16 * 40 * 4
    assert L.daisy_slim_gram_workspace_bytes(100, 40, 32) >= 40 * 40 * 4 + 32 * 40 * 4
    assert L.daisy_slim_gram_fits(10, 40, 0, 1 << 20) == N.DAISY_OK
    assert L.daisy_slim_gram_fits(10, 40000, 0, 1 << 30) == N.DAISY_ERR_ARG
    assert "does not fit the 1073741824 bytes offered" in N.last_error() and "6400000000 bytes" in N.last_error()
    big = 2_000_000_000                                    # G + workspace pass 2^64: refused all the same
    assert L.daisy_slim_gram_fits(10, big, 0, (1 << 64) - 1) == N.DAISY_ERR_ARG and "does not fit" in N.last_error()
    assert L.daisy_slim_gram(None, d, d, 10, 40, d, d, 1 << 20, None) == N.DAISY_ERR_ARG and "NULL" in N.last_error()
    assert L.daisy_slim_gram(d, d, d, 10, 0, d, d, 1 << 20, None) == N.DAISY_ERR_ARG and "item_num" in N.last_error()
    assert L.daisy_slim_gram(d, d, d, 10, 40, d, d, 100, None) == N.DAISY_ERR_ARG and "workspace" in N.last_error()

    def cd(G=d, I=40, n=10, alpha=1.0, l1r=0.1, tol=1e-4, max_iter=100, topk=5, col0=0, ncols=40, path=0, ws=1 << 20):
        return L.daisy_slim_cd(G, I, n, alpha, l1r, tol, max_iter, topk, col0, ncols, d, d, d, d, d, None, path, d, ws, None)
    for kw, msg in ((dict(G=None), "NULL"), (dict(I=0), "item_num"), (dict(alpha=0.0), "alpha"), (dict(alpha=-2.0), "alpha"),
                    (dict(l1r=1.01), "l1_ratio"), (dict(l1r=-0.01), "l1_ratio"), (dict(tol=-1.0), "tol"),
                    (dict(max_iter=0), "max_iter"), (dict(topk=0), "topk"), (dict(topk=N.SLIM_MAX_TOPK + 1), "topk"),
                    (dict(col0=-1), "columns"), (dict(col0=35, ncols=6), "columns"), (dict(path=3), "path"),
                    (dict(I=N.SLIM_LDS_ITEMS + 1, ncols=1, path=1, ws=1 << 30), "LDS path"), (dict(ws=64), "workspace")):
        assert cd(**kw) == N.DAISY_ERR_ARG, kw
        assert msg in N.last_error(), (kw, N.last_error())
    assert L.daisy_slim_cd_workspace_bytes(40, 41, 0) == 0 and L.daisy_slim_cd_workspace_bytes(40, 40, 7) == 0
    lds, glob = L.daisy_slim_cd_workspace_bytes(40, 40, 1), L.daisy_slim_cd_workspace_bytes(40, 40, 2)
    assert lds >= 256 + 160 and glob >= lds + 40 * 2 * 40 * 8
    # state in global memory: at most one workgroup per CU (256)
    assert L.daisy_slim_cd_workspace_bytes(20000, 20000, 2) < 257 * 2 * 20000 * 8 + 20000 * 4 + 1024
    assert L.daisy_slim_cd_workspace_bytes(N.SLIM_LDS_ITEMS + 1, 8, 0) >= 8 * 2 * (N.SLIM_LDS_ITEMS + 1) * 8   # auto: global

    def sc(rp=d, wp=d, out=d, U=10, I=40, users=d, B=4, items=d, Cn=3, path=0, col=d, val=d, wr=d, wv=d):
        return L.daisy_slim_scores(rp, col, val, U, I, wp, wr, wv, users, B, items, Cn, out, path, None)
    for kw, msg in ((dict(rp=None), "NULL"), (dict(wp=None), "NULL"), (dict(out=None), "NULL"), (dict(col=None), "NULL"),
                    (dict(val=None), "NULL"), (dict(wr=None), "NULL"), (dict(wv=None), "NULL"), (dict(I=0), "item_num"),
                    (dict(users=None), "users"), (dict(B=-1), "B="), (dict(Cn=0), "candidates"), (dict(path=-1), "path"),
                    (dict(I=40000, path=1), "LDS path")):
        assert sc(**kw) == N.DAISY_ERR_ARG, kw
        assert msg in N.last_error(), (kw, N.last_error())
