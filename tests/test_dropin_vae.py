"""Multi-VAE on the host: the reference's UNMODIFIED run_examples/test.py and tune.py with --algo_name multi-vae reach
`fit` of daisyrec_amd's VAECF (dropin.install()), which refuses to run without a device (no CPU fallback); the mirror's
initial state and state_dict against the reference under one seed; the item-0 rule of get_user_rating_matrix; the
argument checks of the daisy_vae_* entry points (before any HIP call)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from test_oracle_vae import vae_config

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
def test_reference_driver_reaches_the_hip_vae(tmp_path):
    d = _checkout(tmp_path)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_daisy_example.py"), "--daisy", str(d), "--",
                        "--algo_name", "multi-vae", "--epochs", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "no HIP device visible" in r.stderr, r.stderr[-2000:]
    assert "model.fit(train_loader)" in r.stderr, r.stderr[-2000:]
    assert os.path.join("daisyrec_amd", "model", "VAECFRecommender.py") in r.stderr, r.stderr[-2000:]


@needs_ref
@host_only
def test_reference_tune_driver_reaches_the_hip_vae(tmp_path):
    d = _checkout(tmp_path)
    pack = '{"latent_dim": [64, 128], "lr": {"min": 0.001, "max": 0.01, "step": null}}'
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_daisy_example.py"), "--daisy", str(d),
                        "--script", "run_examples/tune.py",
                        "--extra-path", os.path.join(ROOT, "tests", "golden", "_shims_optuna"), "--",
                        "--algo_name", "multi-vae", "--epochs", "1", "--hyperopt_trail", "1", "--tune_pack", pack],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "no HIP device visible" in r.stderr, r.stderr[-3000:]
    assert "model.fit(train_loader)" in r.stderr and "in objective" in r.stderr, r.stderr[-3000:]
    assert os.path.join("daisyrec_amd", "model", "VAECFRecommender.py") in r.stderr, r.stderr[-3000:]


@needs_ref
def test_init_and_state_dict_equal_the_reference():
    """the same seed gives the reference's parameters, keys and shapes (odd latent_dim and two hidden layers too)"""
    sys.path.insert(0, REF)
    try:
        from daisy.model.VAECFRecommender import VAECF as RefVAECF
    finally:
        sys.path.remove(REF)
    from daisyrec_amd.model import VAECF
    hid = torch.tensor([[1, 2, 0], [3, 0, 0]])
    hval = torch.tensor([[1.0, 1.0, 1.0], [1.0, 0.0, 0.0]])
    for hidden, lat in ((None, 128), ([9], 7), ([12, 10], 6)):
        cfg = vae_config(user_num=2, item_num=5, mlp_hidden_size=hidden, latent_dim=lat, history_item_id=hid,
                         history_item_value=hval)
        torch.manual_seed(3)
        a = RefVAECF(cfg).state_dict()
        torch.manual_seed(3)
        m = VAECF(cfg)
        b = m.state_dict()
        assert list(a) == list(b)
        for k in a:
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
        assert m.decode_layer_dims[0] == lat // 2


def test_item0_rule_of_get_user_rating_matrix():
    """index_put_ without accumulation: the padding (item 0, value 0) after every row shorter than the longest erases
    the row's item 0; the longest row keeps it"""
    from daisyrec_amd.model import VAECF
    hid = torch.tensor([[0, 2, 0], [4, 0, 3], [0, 0, 0]])
    hval = torch.tensor([[1.0, 1.0, 0.0], [1.0, 1.0, 1.0], [1.0, 0.0, 0.0]])
    m = VAECF(vae_config(user_num=3, item_num=5, latent_dim=4, mlp_hidden_size=[3], history_item_id=hid,
                         history_item_value=hval))
    R = m.get_user_rating_matrix(torch.tensor([0, 1, 2]))
    assert R.tolist() == [[0, 0, 1, 0, 0], [1, 0, 0, 1, 1], [0, 0, 0, 0, 0]]
    from daisyrec_amd import ops
    rp, col, val = ops.vae_history_csr(hid, hval, 5)
    assert rp.tolist() == [0, 1, 4, 4] and col.tolist() == [2, 0, 3, 4] and val.tolist() == [1.0] * 4


def test_surface_errors_without_a_device():
    from daisyrec_amd.model import VAECF
    m = VAECF(vae_config(user_num=3, item_num=5, latent_dim=4, mlp_hidden_size=[3],
                         history_item_id=torch.zeros(3, 1, dtype=torch.long), history_item_value=torch.ones(3, 1)))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device visible"):
            m.full_rank(0)
    with pytest.raises(NotImplementedError):
        m.forward(torch.zeros(1, 5))
    with pytest.raises(ValueError, match="latent_dim"):
        VAECF(vae_config(user_num=3, item_num=5, latent_dim=1, history_item_id=torch.zeros(3, 1, dtype=torch.long),
                         history_item_value=torch.ones(3, 1)))


def test_vae_abi_argument_errors():
    from daisyrec_amd import _native as N
    h = ctypes.c_void_p()
    hid = (ctypes.c_int32 * 1)(600)
    assert N.lib.daisy_vae_ctx_create(None, 16, 100, 10, 1, hid, 128) == N.DAISY_ERR_ARG
    assert "NULL" in N.last_error()
    for args, msg in [((0, 100, 10, 1, hid, 128), "max_batch"), ((16, -1, 10, 1, hid, 128), "max_entries"),
                      ((16, 100, 0, 1, hid, 128), "item_num"), ((16, 100, 10, 9, hid, 128), "n_hidden"),
                      ((16, 100, 10, 1, None, 128), "hidden"), ((16, 100, 10, 1, hid, 1), "latent_dim")]:
        assert N.lib.daisy_vae_ctx_create(ctypes.byref(h), *args) == N.DAISY_ERR_ARG, args
        assert msg in N.last_error(), (args, N.last_error())
    assert N.lib.daisy_vae_ctx_destroy(None) == N.DAISY_OK
    assert N.lib.daisy_vae_ctx_bytes(None) == 0
    assert N.lib.daisy_vae_param_count(None) == 0
    assert N.lib.daisy_vae_step_grads(None, None, None, None, None, None, 10, None, 4, 10, None, None, 1, 0.5, 0.0, 0,
                                      None, None) == N.DAISY_ERR_ARG
    assert N.lib.daisy_vae_fit_epoch(None, None, None, None, None, None, 10, None, 8, 4, None, 0.5, 0.2, 100, 0, 0, 0, 0,
                                     1, 1e-3, None, None, None, None) == N.DAISY_ERR_ARG
    assert N.lib.daisy_vae_scores(None, None, None, None, None, 10, None, 4, 10, None, 0, None, None, 0, 0.0, 0, None,
                                  None) == N.DAISY_ERR_ARG
