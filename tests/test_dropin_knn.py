"""ItemKNN / UserKNN on the host: the reference's UNMODIFIED run_examples/test.py with --algo_name itemknn reaches `fit` of
daisyrec_amd's ItemKNNCF (dropin.install()), which refuses to run without a device (no CPU fallback); constructor and
frame errors; the argument checks of the daisy_knn_* entry points (before any HIP call); the byte functions past 2^31."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_oracle_knn import knn_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("DAISY_REFERENCE", "/root/reference")
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "daisy")), reason="reference checkout not present")
host_only = pytest.mark.skipif(torch.cuda.is_available(), reason="host-only check (with a device the run would train)")


@needs_ref
@host_only
def test_reference_driver_reaches_the_hip_itemknn(tmp_path):
    d = tmp_path / "daisy_checkout"                        # writable cwd: the driver writes ./log ./res
    d.mkdir()
    for name in ("daisy", "run_examples", "data"):
        os.symlink(os.path.join(REF, name), d / name)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_daisy_example.py"), "--daisy", str(d), "--",
                        "--algo_name", "itemknn"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "no HIP device visible" in r.stderr, r.stderr[-2000:]
    assert "model.fit(train_set)" in r.stderr, r.stderr[-2000:]
    assert os.path.join("daisyrec_amd", "model", "KNNCFRecommender.py") in r.stderr, r.stderr[-2000:]


def test_dropin_rebinds_both_reference_names():
    if not os.path.isdir(os.path.join(REF, "daisy")):
        pytest.skip("reference checkout not present")
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import daisyrec_amd.dropin as d; d.install()\n"
            "import daisy.model.KNNCFRecommender as m; from daisyrec_amd.model import ItemKNNCF, UserKNNCF\n"
            "assert m.ItemKNNCF is ItemKNNCF and m.UserKNNCF is UserKNNCF\n") % (os.path.join(ROOT, "tests", "golden", "_shims"),
                                                                               REF, ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def _frame(u, i, r, names=("user", "item", "rating")):
    import pandas as pd
    return pd.DataFrame(dict(zip(names, (u, i, r))))


@pytest.mark.parametrize("name", ["ItemKNNCF", "UserKNNCF"])
def test_surface_errors_without_a_device(name):
    import daisyrec_amd.model as models
    cls = getattr(models, name)
    m = cls(knn_config())
    assert (m.k, m.shrink, m.normalize, m.similarity, m.topk, m.user_num, m.item_num) == (40, 100.0, True, "cosine", 10, 3, 4)
    assert m.pred_mat is None and m.w_sparse is None and m.fit_info is None
    with pytest.raises(ValueError, match="'cosine', 'pearson', 'adjusted', 'asymmetric', 'jaccard', 'tanimoto', 'dice', "
                                         "'tversky'. Passed value was 'euclid'"):
        cls(knn_config(similarity="euclid"))
    for sim in ("cosine", "pearson", "adjusted", "asymmetric", "jaccard", "tanimoto", "dice", "tversky"):
        cls(knn_config(similarity=sim))
    for over, msg in ((dict(shrink=-1), "shrink"), (dict(shrink=float("nan")), "shrink"), (dict(shrink=float("inf")), "shrink"),
                      (dict(maxk=0), "maxk"), (dict(topk=0), "topk"), (dict(item_num=0), "item_num"),
                      (dict(user_num=0), "user_num")):
        with pytest.raises(ValueError, match=msg):
            cls(knn_config(**over))
    for frame, msg in ((_frame([0, 3], [0, 1], [1., 1.]), "user id 3"), (_frame([0, 1], [0, 4], [1., 1.]), "item id 4"),
                       (_frame([0, -1], [0, 1], [1., 1.]), "user id -1"), (_frame([0, 1], [0, 1], [1., np.nan]), "finite"),
                       (_frame([0, 1], [0, 1], [1., np.inf]), "finite"), (_frame([0, 0.5], [0, 1], [1., 1.]), "non-integer")):
        with pytest.raises(ValueError, match=msg):
            m.fit(frame)
    # the reference's convert_df reads the literal names, whatever UID_NAME / IID_NAME / INTER_NAME say
    with pytest.raises(KeyError):
        m.fit(_frame([0], [0], [1.]).rename(columns={"rating": "label"}))
    named = cls(knn_config(UID_NAME="uid", IID_NAME="iid", INTER_NAME="click"))
    with pytest.raises(KeyError):
        named.fit(_frame([0], [0], [1.], names=("uid", "iid", "click")))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device visible"):
            m.fit(_frame([0, 1], [0, 1], [1., 1.]))
        with pytest.raises(RuntimeError, match="no HIP device visible"):
            m.full_rank(0)


def test_similarity_plan():
    from daisyrec_amd import ops
    assert ops.knn_plan("cosine", True) == ("none", "cosine", True) and ops.knn_plan("cosine", False) == ("none", "plain", True)
    assert ops.knn_plan("adjusted", True) == ("row", "cosine", True) and ops.knn_plan("pearson", False) == ("col", "plain", True)
    assert ops.knn_plan("asymmetric", True) == ("none", "asymmetric", True)
    for name, mode in (("jaccard", "tanimoto"), ("tanimoto", "tanimoto"), ("dice", "dice"), ("tversky", "tversky")):
        assert ops.knn_plan(name, True) == ops.knn_plan(name, False) == ("binary", mode, False)
    with pytest.raises(ValueError, match="not recognized"):
        ops.knn_plan("euclid", True)


def test_knn_abi_argument_errors():
    from daisyrec_amd import _native as N
    L = N.lib
    buf = ctypes.create_string_buffer(256)
    d = ctypes.addressof(buf)                              # a dummy pointer nobody reads

    def expect(rc, name, msg, what):
        assert rc == N.DAISY_ERR_ARG, what
        assert N.last_error().startswith(name + ":") and msg in N.last_error(), (what, N.last_error())

    # bytes: G, the Gram workspace, count + rows + vals + norms; 64-bit past n^2 > 2^31
    assert L.daisy_knn_fit_bytes(10, 0, 7) == 0 and L.daisy_knn_fit_bytes(-1, 5, 7) == 0
    assert L.daisy_knn_fit_bytes(10, 5, 0) == 0 and L.daisy_knn_fit_bytes(10, 5, N.KNN_MAX_K + 1) == 0
    assert L.daisy_knn_fit_bytes(10, 1 << 40, 7) == 0
    for rows, n, K in ((943, 1682, 40), (1682, 943, 40), (100000, 46341, 1024), (5, 70000, 7)):
        ws = L.daisy_slim_gram_workspace_bytes(rows, n, 0)
        lo = n * n * 4 + ws + n * 4 + 2 * n * K * 4 + n * 4
        got = L.daisy_knn_fit_bytes(rows, n, K)
        assert lo <= got <= lo + 5 * 256, (rows, n, K)
        assert L.daisy_knn_fits(rows, n, K, got) == N.DAISY_OK
        expect(L.daisy_knn_fits(rows, n, K, got - 1), "knn_fits", "does not fit", (rows, n, K))
        assert f"{got} bytes" in N.last_error() and f"{got - 1} bytes offered" in N.last_error()
    assert L.daisy_knn_fit_bytes(100000, 46341, 1024) > 1 << 33
    expect(L.daisy_knn_fits(10, 0, 7, 1 << 30), "knn_fits", "n=", "n")
    expect(L.daisy_knn_fits(-1, 5, 7, 1 << 30), "knn_fits", "n_rows", "n_rows")
    expect(L.daisy_knn_fits(10, 5, 0, 1 << 30), "knn_fits", "K=", "K")
    expect(L.daisy_knn_fits(10, 5, 1025, 1 << 30), "knn_fits", "K=", "K")

    for kw, msg in ((dict(rp=None), "NULL"), (dict(val=None), "NULL"), (dict(mean=None), "NULL"), (dict(R=-1), "n_rows")):
        a = dict(rp=d, val=d, R=4, mean=d)
        a.update(kw)
        expect(L.daisy_knn_row_means(a["rp"], a["val"], a["R"], a["mean"], None), "knn_row_means", msg, kw)
    assert L.daisy_knn_row_means(d, d, 0, d, None) == N.DAISY_OK                     # nothing to do: no launch
    for kw, msg in ((dict(rp=None), "NULL"), (dict(col=None), "NULL"), (dict(val=None), "NULL"), (dict(out=None), "NULL"),
                    (dict(R=-1), "n_rows"), (dict(Cn=0), "n_cols"), (dict(mode=4), "mode"), (dict(mode=-1), "mode"),
                    (dict(mode=1, mean=None), "needs the means"), (dict(mode=2, mean=None), "needs the means")):
        a = dict(rp=d, col=d, val=d, R=4, Cn=5, mode=1, mean=d, out=d)
        a.update(kw)
        expect(L.daisy_knn_center(a["rp"], a["col"], a["val"], a["R"], a["Cn"], a["mode"], a["mean"], a["out"], None),
               "knn_center", msg, kw)
    assert L.daisy_knn_center(d, d, d, 0, 5, 3, None, d, None) == N.DAISY_OK
    for kw, msg in ((dict(G=None), "NULL"), (dict(ss=None), "NULL"), (dict(n=0), "n="), (dict(n=1 << 40), "n=")):
        a = dict(G=d, n=4, ss=d)
        a.update(kw)
        expect(L.daisy_knn_diag(a["G"], a["n"], 1, a["ss"], None), "knn_diag", msg, kw)

    def select(G=d, ss=d, n=40, mode=0, shrink=100.0, alpha=0.5, K=7, count=d, rows=d, vals=d):
        return L.daisy_knn_select(G, ss, n, mode, shrink, alpha, K, count, rows, vals, None)
    for kw, msg in ((dict(G=None), "NULL"), (dict(ss=None), "NULL"), (dict(count=None), "NULL"), (dict(rows=None), "NULL"),
                    (dict(vals=None), "NULL"), (dict(n=0), "n="), (dict(n=1 << 40), "n="), (dict(mode=6), "mode"),
                    (dict(mode=-1), "mode"), (dict(shrink=-1.0), "shrink"), (dict(shrink=float("nan")), "shrink"),
                    (dict(shrink=float("inf")), "shrink"), (dict(alpha=1.5), "alpha"), (dict(alpha=float("nan")), "alpha"),
                    (dict(K=0), "K="), (dict(K=1025), "K=")):
        expect(select(**kw), "knn_select", msg, kw)

    def rank(lp=d, lc=d, lv=d, nr=10, inner=40, rp=d, rr=d, rv=d, nc=40, users=d, B=4, items=d, Cn=3, topk=2, scores=d,
             ids=d, path=0):
        return L.daisy_knn_rank(lp, lc, lv, nr, inner, rp, rr, rv, nc, users, B, items, Cn, topk, scores, ids, path, None)
    for kw, msg in ((dict(lp=None), "NULL"), (dict(lc=None), "NULL"), (dict(lv=None), "NULL"), (dict(rp=None), "NULL"),
                    (dict(rr=None), "NULL"), (dict(rv=None), "NULL"), (dict(scores=None), "NULL"), (dict(nr=0), "n_rows"),
                    (dict(inner=0), "inner"), (dict(nc=0), "n_cols"), (dict(users=None), "users"), (dict(B=-1), "B="),
                    (dict(Cn=0), "candidates"), (dict(items=None, Cn=3), "candidates"), (dict(topk=0), "topk"),
                    (dict(topk=4), "topk"), (dict(path=3), "path"), (dict(path=1, inner=40000), "LDS path")):
        expect(rank(**kw), "knn_rank", msg, kw)
    assert rank(B=0) == N.DAISY_OK                          # nothing to do: no launch
