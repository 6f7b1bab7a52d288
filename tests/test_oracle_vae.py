"""Multi-VAE on the host: the mirror's modules against the REAL reference's initial state (tests/golden/kat_vae.npz), the
mirror's rating rows (the item-0 rule), and the float64 oracle (tests/vae_oracle.py) against the reference's step KATs -
what the GPU tests then hold the kernels to."""
import hashlib
import os

import numpy as np
import pytest
import torch

import vae_oracle as VO
from conftest import mf_config

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["vae_adam", "vae_sgd", "vae_adagrad", "vae_rmsprop_odd"]


def vae_config(**over):
    """test.py's config for --algo_name multi-vae (basic.yaml <- multi-vae.yaml)"""
    cfg = mf_config(algo_name="multi-vae", mlp_hidden_size=None, epochs=10, dropout=0.5, lr=0.001, latent_dim=128,
                    total_anneal_steps=100000, anneal_cap=0.2)
    cfg.update(over)
    return cfg


def kat_model(kat, name, **over):
    """the mirror built like the KAT's reference model (same seed, same config): its initial state"""
    from daisyrec_amd.model import VAECF
    U, I, lat, B, ns, seed, total = (int(x) for x in kat[f"{name}/meta"])
    lr, p, cap = (float(x) for x in kat[f"{name}/hyper"])
    hidden = [int(x) for x in kat[f"{name}/hidden"]]
    torch.manual_seed(seed)
    return VAECF(vae_config(user_num=U, item_num=I, mlp_hidden_size=hidden or None, latent_dim=lat, lr=lr, dropout=p,
                            anneal_cap=cap, total_anneal_steps=total, optimizer=str(kat[f"{name}/optimizer"]),
                            history_item_id=torch.from_numpy(kat[f"{name}/hist_id"]),
                            history_item_value=torch.from_numpy(kat[f"{name}/hist_val"]), **over))


def kat_steps(kat, name):
    ns = int(kat[f"{name}/meta"][4])
    return [(kat[f"{name}/R"][k], kat[f"{name}/keep{k}"], kat[f"{name}/eps{k}"]) for k in range(ns)]


def close(a, b, rtol=1e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(1.0, float(np.abs(b).max())) if b.size else 1.0
    return np.abs(a - b).max(initial=0.0) <= rtol * scale


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(HERE, "golden", "kat_vae.npz"))


def test_init_state_dict_bitwise(kat):
    from daisyrec_amd.model import VAECF
    hid, hval = torch.from_numpy(kat["init_hist_id"]), torch.from_numpy(kat["init_hist_val"])
    for name in kat["init_names"]:
        U, I, lat, seed = (int(x) for x in kat[f"{name}/meta"])
        hidden = [int(x) for x in kat[f"{name}/hidden"]]
        torch.manual_seed(seed)
        m = VAECF(vae_config(user_num=U, item_num=I, mlp_hidden_size=hidden or None, latent_dim=lat, history_item_id=hid,
                             history_item_value=hval))
        sd = m.state_dict()
        assert list(sd.keys()) == list(kat[f"{name}/keys"]), name
        for k, v in sd.items():
            if f"{name}/sha/{k}" in kat:
                assert list(v.shape) == list(kat[f"{name}/shape/{k}"]), (name, k)
                assert hashlib.sha256(v.numpy().tobytes()).hexdigest() == str(kat[f"{name}/sha/{k}"]), (name, k)
            else:
                np.testing.assert_array_equal(v.numpy(), kat[f"{name}/p/{k}"], err_msg=f"{name} {k}")
        assert m.encode_layer_dims == [I] + (hidden or [600]) + [lat]
        assert m.decode_layer_dims == [lat // 2] + (hidden or [600])[::-1] + [I]
        assert m.update == 0 and m.optimizer == "adam" and m.initializer == "xavier_normal"


@pytest.mark.parametrize("case", CASES)
def test_rating_rows_match_reference(kat, case):
    """get_user_rating_matrix: the padding erases item 0 of every row shorter than the longest (last write wins)"""
    m = kat_model(kat, case)
    for k in range(int(kat[f"{case}/meta"][4])):
        R = m.get_user_rating_matrix(torch.from_numpy(kat[f"{case}/users"][k]))
        np.testing.assert_array_equal(R.numpy(), kat[f"{case}/R"][k])
    hid = kat[f"{case}/hist_id"]
    assert (hid[1] == 0).sum() > 1 and hid[3].min() >= 0                  # user 1: item 0 and padding
    R0 = m.get_user_rating_matrix(torch.tensor([1, 2, 3]))
    assert R0[0, 0] == 0 and float(R0[1].abs().sum()) == 0.0 and R0[2, 0] == 1.0


def test_history_csr_matches_rating_rows(kat):
    from daisyrec_amd import ops
    for case in CASES:
        U, I = (int(x) for x in kat[f"{case}/meta"][:2])
        rp, col, val = ops.vae_history_csr(torch.from_numpy(kat[f"{case}/hist_id"]),
                                           torch.from_numpy(kat[f"{case}/hist_val"]), I)
        m = kat_model(kat, case)
        R = m.get_user_rating_matrix(torch.arange(U))
        dense = torch.zeros(U, I)
        for u in range(U):
            lo, hi = int(rp[u]), int(rp[u + 1])
            assert bool((col[lo + 1:hi] > col[lo:hi - 1]).all())          # items ascending within a row
            dense[u, col[lo:hi].long()] = val[lo:hi]
        np.testing.assert_array_equal(dense.numpy(), R.numpy())
        assert bool((val != 0).all())


@pytest.mark.parametrize("case", CASES)
def test_oracle_matches_reference_kats(kat, case):
    U, I, lat, B, ns, seed, total = (int(x) for x in kat[f"{case}/meta"])
    lr, p, cap = (float(x) for x in kat[f"{case}/hyper"])
    m = kat_model(kat, case)
    state = {k: v.numpy() for k, v in m.state_dict().items()}
    losses, params = VO.run_steps(state, kat_steps(kat, case), lat, str(kat[f"{case}/optimizer"]), lr, p, cap, total)
    np.testing.assert_allclose(losses, kat[f"{case}/loss"], rtol=1e-5)
    for k, v in params.items():
        ref = kat[f"{case}/final/p/{k}"]
        upd_ref, upd = ref - state[k], v.numpy() - state[k]
        assert close(upd, upd_ref, 1e-3) or close(v.numpy(), ref, 1e-5), (case, k, np.abs(upd - upd_ref).max())
    assert int(kat[f"{case}/update"]) == ns


def test_ml100k_golden_is_consistent():
    ml = np.load(os.path.join(HERE, "golden", "kat_vae_ml100k.npz"))
    U, I, lat, B = (int(x) for x in ml["ml/meta"][:4])
    nb = int(ml["ml/n_batches"])
    assert ml["ml/hist_len"].shape == (U,) and int(ml["ml/hist_len"].sum()) == ml["ml/hist_items"].size
    per_epoch = nb // 2
    assert nb == 2 * per_epoch and ml["ml/batch_losses"].size == nb
    ep = [np.concatenate([ml[f"ml/users{k}"] for k in range(e * per_epoch, (e + 1) * per_epoch)]) for e in (0, 1)]
    assert sorted(ep[0]) == sorted(ep[1]) and len(set(ep[0])) == ep[0].size        # every training user once per epoch
    assert set(ep[0]) == set(np.nonzero(ml["ml/hist_len"])[0])
    np.testing.assert_allclose(ml["ml/epoch_losses"], [ml["ml/batch_losses"][:per_epoch].sum(),
                                                       ml["ml/batch_losses"][per_epoch:].sum()], rtol=1e-6)
    for k in range(nb):
        assert ml[f"ml/eps{k}"].shape == (ml[f"ml/users{k}"].size, lat // 2)
