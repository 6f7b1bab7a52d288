"""NGCF on the host: the float64 oracle (tests/ngcf_oracle.py) against the golden vectors of the REAL reference NGCF
(tests/golden/kat_ngcf.npz), and the argument checks of the NGCF entry points (no device needed)."""
import ctypes
import os

import numpy as np
import pytest

import ngcf_oracle as NO
from test_oracle_neumf import assert_params_close

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(HERE, "golden", "kat_ngcf.npz"))


def params(g, prefix):
    p = f"{prefix}/p/"
    return {k[len(p):]: g[k] for k in g.files if k.startswith(p)}


def widths(g, name):
    return [int(g[f"{name}/meta"][2])] + [int(x) for x in g[f"{name}/hidden"]]


def test_golden_file_shape(kat):
    assert os.path.getsize(os.path.join(HERE, "golden", "kat_ngcf.npz")) <= 1 << 20
    names = [str(n) for n in kat["names"]]
    hidden = {tuple(int(x) for x in kat[f"{n}/hidden"]) for n in names}
    factors = {int(kat[f"{n}/meta"][2]) for n in names}
    assert {(64, 64, 64), (32, 16), (20,)} <= hidden and {36, 64, 20} <= factors
    keys = [str(k) for k in kat["rank/keys"]]
    assert keys[:4] == ["embed_user.weight", "embed_item.weight", "gnn_layers.0.linear.weight", "gnn_layers.0.linear.bias"]
    assert "gnn_layers.1.interact_transform.bias" in keys


@pytest.mark.parametrize("name", ["ng_bpr_adam", "ng_bpr_adam_reg", "ng_bpr_sgd", "ng_tl_sgd", "ng_cl_adam_reg"])
def test_oracle_reproduces_the_step_kats(kat, name):
    g = kat
    U, I, f, B, ns, _ = (int(x) for x in g[f"{name}/meta"])
    lr, r1, r2 = (float(x) for x in g[f"{name}/hyper"])
    graph = NO.adj(g[f"{name}/gu"], g[f"{name}/gi"], U, I)
    batches = [(g[f"{name}/u"][s], g[f"{name}/i"][s], g[f"{name}/j"][s]) for s in range(ns)]
    opt = str(g[f"{name}/optimizer"])
    losses, p = NO.run_steps(graph, params(g, f"{name}/init"), widths(g, name), batches, str(g[f"{name}/loss_type"]),
                             r1, r2, opt, lr)
    np.testing.assert_allclose(losses, g[f"{name}/loss"], rtol=1e-5)
    want = params(g, f"{name}/final")
    assert set(p) == set(want)
    assert_params_close(p, want, sorted(want), name, 5e-6, adam_lr=lr if opt == "adam" else None, steps=ns, frac=0.98)


def test_oracle_forward_is_the_restored_embeddings(kat):
    g = kat
    U, I, f = (int(x) for x in g["rank/meta"])
    graph = NO.adj(g["rank/gu"], g["rank/gi"], U, I)
    out, _ = NO.forward(graph, params(g, "rank"), widths(g, "rank"))
    out = out.numpy()
    np.testing.assert_allclose(out[:U], g["rank/restore_user"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(out[U:], g["rank/restore_item"], rtol=1e-5, atol=1e-6)


def test_ngcf_argument_errors_do_not_need_a_gpu():
    from daisyrec_amd import _native as N
    lib = N.lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd = lambda n, di, do, mp, E=p, lde=None, ldy=None: lib.daisy_ngcf_layer_forward(  # noqa: E731
        E, di if lde is None else lde, p, p, p, p, p, p, do if ldy is None else ldy, p, n, di, do, mp, 0, 0, None)
    for di, do in [(0, 64), (64, 0), (257, 64), (64, 257), (-1, 8)]:
        assert fwd(10, di, do, 0.0) == N.DAISY_ERR_ARG, (di, do)
        assert "widths" in N.last_error()
    assert fwd(0, 8, 8, 0.0) == N.DAISY_ERR_ARG
    assert fwd(10, 8, 8, 0.0, E=None) == N.DAISY_ERR_ARG and "NULL" in N.last_error()
    assert fwd(10, 8, 8, 0.0, lde=4) == N.DAISY_ERR_ARG and "pitch" in N.last_error()
    for bad_p in (1.0, -0.1, 1.5, float("nan")):
        assert fwd(10, 8, 8, bad_p) == N.DAISY_ERR_ARG and "mess_p" in N.last_error()
    bwd = lambda di, do, mp, dY=p, dE=ctypes.c_void_p(16), ws=p: lib.daisy_ngcf_layer_backward(  # noqa: E731
        dY, do, p, do, p, p, di, p, p, p, None, 0, dE, ctypes.c_void_p(32), ws, 10, di, do, mp, 0, 0, None)
    assert bwd(300, 8, 0.0) == N.DAISY_ERR_ARG and "widths" in N.last_error()
    assert bwd(8, 8, 0.0, ws=None) == N.DAISY_ERR_ARG and "NULL" in N.last_error()
    assert bwd(8, 8, 0.0, dE=p) == N.DAISY_ERR_ARG and "distinct" in N.last_error()
    assert bwd(8, 8, 1.0) == N.DAISY_ERR_ARG and "mess_p" in N.last_error()
    assert lib.daisy_ngcf_wgrad_reduce(p, 10, 8, 0, p, p, p, p, None) == N.DAISY_ERR_ARG
    assert lib.daisy_ngcf_wgrad_reduce(None, 10, 8, 8, p, p, p, p, None) == N.DAISY_ERR_ARG
    assert lib.daisy_ngcf_ws_bytes(10, 8, 300) == 0 and lib.daisy_ngcf_ws_bytes(10, 8, 8) > 10 * 8 * 4
    assert lib.daisy_dropout_mask(0, 1, 10, 1.0, p, None) == N.DAISY_ERR_ARG and "p=" in N.last_error()
    assert lib.daisy_dropout_mask(0, 1, 10, 0.5, None, None) == N.DAISY_ERR_ARG
    assert lib.daisy_lgcn_spmm_ex(None, p, 8, ctypes.c_void_p(16), 8, 8, 0, 0.0, 0, 0, None) == N.DAISY_ERR_ARG
    assert N.ABI_VERSION == 8 == lib.daisy_abi_version()


def test_ngcf_class_is_exported_and_checks_widths():
    from daisyrec_amd.model import NGCF
    from daisyrec_amd.model.NGCFRecommender import BiGNN
    assert NGCF.__name__ == "NGCF" and BiGNN(3, 4).interact_transform.weight.shape == (4, 3)
