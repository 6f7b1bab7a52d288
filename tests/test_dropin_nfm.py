"""NFM on the host: the reference's UNMODIFIED run_examples/test.py and tune.py with --algo_name nfm reach `fit` of
daisyrec_amd's NFM (dropin.install()), which refuses to run without a device (no CPU fallback); the mirror's surface
errors; the argument checks of the daisy_nfm_* entry points (before any HIP call)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from test_oracle_nfm import nfm_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("DAISY_REFERENCE", "/root/reference")
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "daisy")), reason="reference checkout not present")
host_only = pytest.mark.skipif(torch.cuda.is_available(), reason="host-only check (with a device the run would train)")


def _checkout(tmp_path):
    d = tmp_path / "daisy_checkout"                        # writable cwd: the drivers write ./log ./res
    d.mkdir()
    for name in ("daisy", "run_examples", "data"):
        os.symlink(os.path.join(REF, name), d / name)
    return d


@needs_ref
@host_only
def test_reference_driver_reaches_the_hip_nfm(tmp_path):
    d = _checkout(tmp_path)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_daisy_example.py"), "--daisy", str(d), "--",
                        "--algo_name", "nfm", "--epochs", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "no HIP device visible" in r.stderr, r.stderr[-2000:]
    assert "model.fit(train_loader)" in r.stderr, r.stderr[-2000:]
    assert os.path.join("daisyrec_amd", "model", "NFMRecommender.py") in r.stderr, r.stderr[-2000:]


@needs_ref
@host_only
def test_reference_tune_driver_reaches_the_hip_nfm(tmp_path):
    d = _checkout(tmp_path)
    pack = '{"factors": [16, 32], "lr": {"min": 0.01, "max": 0.05, "step": null}, "num_ng": {"min": 1, "max": 2, "step": 1}}'
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_daisy_example.py"), "--daisy", str(d),
                        "--script", "run_examples/tune.py",
                        "--extra-path", os.path.join(ROOT, "tests", "golden", "_shims_optuna"), "--",
                        "--algo_name", "nfm", "--epochs", "1", "--hyperopt_trail", "1", "--tune_pack", pack],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "no HIP device visible" in r.stderr, r.stderr[-3000:]
    assert "model.fit(train_loader)" in r.stderr and "in objective" in r.stderr, r.stderr[-3000:]
    assert os.path.join("daisyrec_amd", "model", "NFMRecommender.py") in r.stderr, r.stderr[-3000:]


def test_predict_and_one_row_errors():
    from daisyrec_amd.model import NFM
    m = NFM(nfm_config(user_num=5, item_num=6, factors=4))
    with pytest.raises(ValueError, match="expected 2D or 3D input"):
        m.predict(1, 2)
    m.train()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        m._one_row_check(1)
    m.eval()
    m._one_row_check(1)                       # eval mode: running statistics, one row is fine
    with pytest.raises(ValueError, match="factors"):
        NFM(nfm_config(user_num=5, item_num=6, factors=257))


def test_nfm_abi_argument_errors():
    from daisyrec_amd import _native as N
    h = ctypes.c_void_p()
    assert N.lib.daisy_nfm_ctx_create(None, 16, 30, 2, 1, 1, 10, 10) == N.DAISY_ERR_ARG
    assert "NULL" in N.last_error()
    for args, msg in [((0, 30, 2, 1, 1, 10, 10), "max_rows"), ((16, 0, 2, 1, 1, 10, 10), "factors"),
                      ((16, 257, 2, 1, 1, 10, 10), "factors"), ((16, 30, 9, 1, 1, 10, 10), "num_layers"),
                      ((16, 30, 2, 7, 1, 10, 10), "act"), ((16, 30, 2, 1, 1, 0, 10), "user_num")]:
        assert N.lib.daisy_nfm_ctx_create(ctypes.byref(h), *args) == N.DAISY_ERR_ARG, args
        assert msg in N.last_error(), (args, N.last_error())
    assert N.lib.daisy_nfm_ctx_destroy(None) == N.DAISY_OK
    assert N.lib.daisy_nfm_ctx_bytes(None) == 0
    p = N.NfmParams()
    assert N.lib.daisy_nfm_step_grads(None, ctypes.byref(p), ctypes.byref(p), None, None, None, None, 4, 0, 1e-10, 0.0,
                                      0.0, 0.0, 0, None, None) == N.DAISY_ERR_ARG
    assert N.lib.daisy_nfm_scores(None, ctypes.byref(p), None, None, None, 4, 0, 0, 0.0, 0, None, None) == N.DAISY_ERR_ARG
    assert N.lib.daisy_nfm_fit_epoch(None, ctypes.byref(p), ctypes.byref(p), None, None, None, None, 4, 2, 0, 1e-10, 0.0,
                                     0.0, 0.0, 0, 0, 0, 0, 0.01, None, None, None, None, 10, None, None) == N.DAISY_ERR_ARG
    assert N.lib.daisy_nfm_ctx_set_path(None, 1) == N.DAISY_ERR_ARG
