"""NFM on the host: the mirror's modules against the REAL reference's initial state (tests/golden/kat_nfm.npz), and the
float64 oracle (tests/nfm_oracle.py) against the reference's step KATs - what the GPU tests then hold the kernels to."""
import os

import numpy as np
import pytest
import torch

import nfm_oracle as NO
from conftest import mf_config

HERE = os.path.dirname(os.path.abspath(__file__))


def nfm_config(**over):
    """test.py's config for --algo_name nfm (basic.yaml <- nfm.yaml)"""
    cfg = mf_config(algo_name="nfm", factors=30, act_function="relu", num_layers=2, batch_norm=True, dropout=0.5,
                    epochs=30, lr=1e-3, reg_1=0.0, reg_2=0.0)
    cfg.update(over)
    return cfg


def kat_model(kat, name, **over):
    """the mirror built like the KAT's reference model (same seed, same config): its initial state"""
    from daisyrec_amd.model import NFM
    U, I, f, L, bn, B, ns, seed = (int(x) for x in kat[f"{name}/meta"])
    lr, r1, r2 = (float(x) for x in kat[f"{name}/hyper"])
    torch.manual_seed(seed)
    return NFM(nfm_config(user_num=U, item_num=I, factors=f, num_layers=L, batch_norm=bool(bn),
                          act_function=str(kat[f"{name}/act"]), dropout=0.0, loss_type=str(kat[f"{name}/loss_type"]),
                          optimizer=str(kat[f"{name}/optimizer"]), lr=lr, reg_1=r1, reg_2=r2, **over))


def close(a, b, rtol=1e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(1.0, float(np.abs(b).max())) if b.size else 1.0
    return np.abs(a - b).max(initial=0.0) <= rtol * scale


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(HERE, "golden", "kat_nfm.npz"))


def test_init_state_dict_bitwise(kat):
    from daisyrec_amd.model import NFM
    for name in kat["init_names"]:
        U, I, f, L, bn, seed = (int(x) for x in kat[f"{name}/meta"])
        torch.manual_seed(seed)
        m = NFM(nfm_config(user_num=U, item_num=I, factors=f, num_layers=L, batch_norm=bool(bn),
                           act_function=str(kat[f"{name}/act"])))
        sd = m.state_dict()
        assert list(sd.keys()) == list(kat[f"{name}/keys"]), name
        for k, v in sd.items():
            np.testing.assert_array_equal(v.numpy(), kat[f"{name}/p/{k}"], err_msg=f"{name} {k}")


@pytest.mark.parametrize("case", ["nf_bpr_sgd", "nf_bpr_sgd_nobn", "nf_bpr_adam_reg", "nf_hl_sgd_reg", "nf_tl_adam",
                                  "nf_cl_sgd_reg", "nf_cl_adam", "nf_sl_sgd", "nf_sl_adam_reg_nobn",
                                  "nf_bpr_adam_L0_nobn", "nf_hl_adam_other"])
def test_oracle_matches_reference_kats(kat, case):
    U, I, f, L, bn, B, ns, seed = (int(x) for x in kat[f"{case}/meta"])
    lr, r1, r2 = (float(x) for x in kat[f"{case}/hyper"])
    m = kat_model(kat, case)
    state = {k: v.numpy() for k, v in m.state_dict().items()}
    steps = [(kat[f"{case}/u"][k], kat[f"{case}/i"][k], kat[f"{case}/j"][k]) for k in range(ns)]
    losses, params, bufs = NO.run_steps(state, steps, L, bool(bn), str(kat[f"{case}/act"]), str(kat[f"{case}/loss_type"]),
                                        str(kat[f"{case}/optimizer"]), lr, r1, r2)
    np.testing.assert_allclose(losses, kat[f"{case}/loss"], rtol=1e-5)
    skip = NO.zero_grad_params(state, L, bool(bn)) if str(kat[f"{case}/optimizer"]) == "adam" else set()
    for k, v in {**params, **bufs}.items():
        ref = kat[f"{case}/final/p/{k}"]
        if k in skip:
            continue
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(ref), k
        else:
            assert close(v.numpy(), ref, 1e-4), (case, k, np.abs(v.numpy() - ref).max())
