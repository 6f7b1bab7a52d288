"""PureSVD on the host: the reference's UNMODIFIED run_examples/test.py with --algo_name puresvd reaches `fit` of
daisyrec_amd's PureSVD (dropin.install()), which refuses to run without a device (no CPU fallback); constructor and
DataFrame errors; the argument checks of the daisy_psvd_* entry points (before any HIP call)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_oracle_puresvd import puresvd_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("DAISY_REFERENCE", "/root/reference")
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "daisy")), reason="reference checkout not present")
host_only = pytest.mark.skipif(torch.cuda.is_available(), reason="host-only check (with a device the run would fit)")


@needs_ref
@host_only
def test_reference_driver_reaches_the_hip_puresvd(tmp_path):
    d = tmp_path / "daisy_checkout"                        # writable cwd: the driver writes ./log ./res
    d.mkdir()
    for name in ("daisy", "run_examples", "data"):
        os.symlink(os.path.join(REF, name), d / name)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_daisy_example.py"), "--daisy", str(d), "--",
                        "--algo_name", "puresvd"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "no HIP device visible" in r.stderr, r.stderr[-2000:]
    assert "model.fit(train_set)" in r.stderr, r.stderr[-2000:]
    assert os.path.join("daisyrec_amd", "model", "PureSVDRecommender.py") in r.stderr, r.stderr[-2000:]


def test_dropin_rebinds_the_reference_name():
    if not os.path.isdir(os.path.join(REF, "daisy")):
        pytest.skip("reference checkout not present")
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import daisyrec_amd.dropin as d; d.install()\n"
            "import daisy.model.PureSVDRecommender as m; from daisyrec_amd.model import PureSVD\n"
            "assert m.PureSVD is PureSVD\n") % (os.path.join(ROOT, "tests", "golden", "_shims"), REF, ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def _frame(u, i, r):
    import pandas as pd
    return pd.DataFrame({"user": u, "item": i, "rating": r})


def test_surface_errors_without_a_device():
    from daisyrec_amd.model import PureSVD
    m = PureSVD(puresvd_config())
    assert (m.user_num, m.item_num, m.factors, m.topk, m.max_sweeps) == (3, 4, 2, 10, 60)
    assert m.user_vec is None and m.item_vec is None and m.fit_info is None
    assert PureSVD(puresvd_config(factors=246)).factors == 246
    for over, msg in ((dict(factors=0), "factors"), (dict(factors=-3), "factors"), (dict(factors=247), "factors"),
                      (dict(topk=0), "topk"), (dict(item_num=0), "item_num"), (dict(user_num=-1), "user_num")):
        with pytest.raises(ValueError, match=msg):
            PureSVD(puresvd_config(**over))
    for frame, msg in ((_frame([0, 3], [0, 1], [1., 1.]), r"PureSVD.fit: user id 3"),
                       (_frame([0, 1], [0, 4], [1., 1.]), r"PureSVD.fit: item id 4"),
                       (_frame([0, -1], [0, 1], [1., 1.]), r"PureSVD.fit: user id -1"),
                       (_frame([0, 1.5], [0, 1], [1., 1.]), r"PureSVD.fit: column 'user' holds non-integer"),
                       (_frame([0, 1], [0, 1], [1., np.inf]), r"PureSVD.fit: column 'rating'.*finite")):
        with pytest.raises(ValueError, match=msg):
            m.fit(frame)
    with pytest.raises(KeyError):
        m.fit(_frame([0], [0], [1.]).rename(columns={"rating": "label"}))
    if not torch.cuda.is_available():
        for call in (lambda: m.fit(_frame([0, 1], [0, 1], [1., 1.])), lambda: m.full_rank(0), lambda: m.predict(0, 0),
                     lambda: m.rank([])):
            with pytest.raises(RuntimeError, match="no HIP device visible"):
                call()


def test_psvd_abi_argument_errors():
    from daisyrec_amd import _native as N
    L = N.lib
    buf = ctypes.create_string_buffer(256)
    d = ctypes.addressof(buf)                              # a dummy pointer nobody reads
    big = N.PSVD_MAX_C + 1

    def errs(fn, defaults, cases):
        for kw, msg in cases:
            a = dict(defaults)
            a.update(kw)
            assert fn(**a) == N.DAISY_ERR_ARG, kw
            assert msg in N.last_error(), (kw, N.last_error())

    def spmm(rp=d, col=d, val=d, n=5, m=4, X=d, c=3, Y=d):
        return L.daisy_psvd_spmm(rp, col, val, n, m, X, c, Y, None)
    errs(spmm, {}, ((dict(rp=None), "NULL"), (dict(col=None), "NULL"), (dict(val=None), "NULL"), (dict(X=None), "NULL"),
                    (dict(Y=None), "NULL"), (dict(c=big), "c=257"), (dict(c=0), "c=0"), (dict(n=-1), "n_rows=-1"),
                    (dict(m=0), "n_cols=0")))

    assert L.daisy_psvd_gram_block_rows(1000, 0) == 256 and L.daisy_psvd_gram_block_rows(1000, 333) == 336
    assert L.daisy_psvd_gram_block_rows(1 << 20, 0) == 4096 and L.daisy_psvd_gram_block_rows(0, 0) == 0
    assert L.daisy_psvd_gram_workspace_bytes(1000, 26, 0) >= 4 * 26 * 26 * 8
    assert L.daisy_psvd_gram_workspace_bytes(1000, big, 0) == 0 and L.daisy_psvd_gram_workspace_bytes(0, 26, 0) == 0

    def gram(Y=d, n=1000, c=26, G=d, rows=0, ws=d, nbytes=1 << 20):
        return L.daisy_psvd_gram(Y, n, c, G, rows, ws, nbytes, None)
    errs(gram, {}, ((dict(Y=None), "NULL"), (dict(G=None), "NULL"), (dict(ws=None), "NULL"), (dict(c=big), "c=257"),
                    (dict(n=0), "n=0"), (dict(n=-4), "n=-4"), (dict(nbytes=4 * 26 * 26 * 8 - 1), "workspace"),
                    (dict(n=1 << 20, rows=4, nbytes=1 << 40), "blocks")))

    def chol(G=d, c=26, n=100, R=d, Ri=d, dropped=d):
        return L.daisy_psvd_chol(G, c, n, R, Ri, dropped, None)
    errs(chol, {}, ((dict(G=None), "NULL"), (dict(R=None), "NULL"), (dict(Ri=None), "NULL"), (dict(dropped=None), "NULL"),
                    (dict(c=big), "c=257"), (dict(c=0), "c=0"), (dict(n=0), "n=0"), (dict(n=-1), "n=-1")))

    def gemm(Y=d, T=d, C=d, n=100, c=26, c2=26):
        return L.daisy_psvd_gemm(Y, T, C, n, c, c2, None)
    errs(gemm, {}, ((dict(Y=None), "NULL"), (dict(T=None), "NULL"), (dict(C=None), "NULL"), (dict(n=-1), "n=-1"),
                    (dict(c=big), "c=257"), (dict(c2=big), "c2=257"), (dict(c2=0), "c2=0")))

    assert L.daisy_psvd_jacobi_workspace_bytes(256) >= 2 * 256 * 256 * 8 and L.daisy_psvd_jacobi_workspace_bytes(big) == 0

    def jacobi(A=d, c=26, sweeps=60, U=d, s=d, V=d, info=d, ws=d, nbytes=1 << 20):
        return L.daisy_psvd_jacobi(A, c, sweeps, U, s, V, info, ws, nbytes, None)
    errs(jacobi, {}, ((dict(A=None), "NULL"), (dict(U=None), "NULL"), (dict(s=None), "NULL"), (dict(V=None), "NULL"),
                      (dict(info=None), "NULL"), (dict(ws=None), "NULL"), (dict(c=big), "c=257"), (dict(c=-1), "c=-1"),
                      (dict(sweeps=0), "max_sweeps=0"), (dict(sweeps=-5), "max_sweeps=-5"),
                      (dict(nbytes=2 * 26 * 26 * 8 - 1), "workspace")))

    def rank(uv=d, iv=d, U=10, I=40, k=8, users=d, B=4, items=d, Cn=30, topk=10, scores=d, ids=d):
        return L.daisy_psvd_rank(uv, iv, U, I, k, users, B, items, Cn, topk, scores, ids, None)
    errs(rank, {}, ((dict(uv=None), "NULL"), (dict(iv=None), "NULL"), (dict(scores=None), "NULL"), (dict(U=0), "user_num=0"),
                    (dict(I=-2), "item_num=-2"), (dict(k=big), "k=257"), (dict(k=0), "k=0"), (dict(users=None), "users"),
                    (dict(B=-1), "B=-1"), (dict(Cn=0), "C=0"), (dict(items=None, Cn=30), "C=30"), (dict(topk=0), "topk=0"),
                    (dict(topk=31), "topk=31")))
    assert rank(B=0) == N.DAISY_OK
