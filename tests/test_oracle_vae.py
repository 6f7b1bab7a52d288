"""Multi-VAE on the host: the mirror's modules against the REAL reference's initial state (tests/golden/kat_vae.npz), the
mirror's rating rows (the item-0 rule), and the float64 oracle (tests/vae_oracle.py) against the reference's step KATs -
what the GPU tests then hold the kernels to."""
import hashlib
import os

import numpy as np
import pytest
import torch

import vae_cases as VC
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
        np.testing.assert_array_equal(R.cpu().numpy(), kat[f"{case}/R"][k])
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
        np.testing.assert_array_equal(dense.numpy(), R.cpu().numpy())
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


@pytest.mark.parametrize("name", VC.NAMES)
def test_edge_cases_hold_their_promises_and_the_fp32_restatement_agrees(name):
    """tests/vae_cases.py before any device sees it: every case has the structure its kernel path needs, the model's
    rating rows and CSR of its history arrays are its R (item 0 stays out, so the padding rule changes nothing), and the
    oracle's code run in torch.float32 - the reference's own arithmetic - holds the bounds the kernels are held to
    (loss 1e-5 relative, every gradient 1e-5 of its tensor's largest element)."""
    from daisyrec_amd import ops
    from daisyrec_amd.model import VAECF
    c = VC.case(name)
    R, lens = c.R, (c.R != 0).sum(1)
    assert R.shape == (c.B, c.I) and R.dtype == np.float64 and not R[:, 0].any()
    assert c.keep.dtype == np.uint8 and c.keep.size == int(lens.sum()) and 0 < int(c.keep.sum()) < c.keep.size
    assert c.eps.shape == (c.B, c.lat // 2) and c.eps.dtype == np.float32
    assert (c.p, c.anneal) == (0.5, 0.2)
    layers = VO.linear_names(c.state, "encoder") + VO.linear_names(c.state, "decoder")
    assert len(layers) == 2 * (len(c.hidden) + 1) and all(c.state[k].dtype == np.float32 for wb in layers for k in wb)
    d1 = (c.hidden + [c.lat])[0]
    assert c.state["encoder.0.weight"].shape == (d1, c.I)
    assert (d1 % 4 == 0) == name.endswith("_v4") or name == "hot_softmax"       # the kernel form the name promises
    if name.startswith("wide_"):
        assert 1024 < d1 <= 2048 and d1 - 1024 == (3 if name == "wide_scalar" else 4)
    if name.startswith("nohidden_"):
        assert c.hidden == [] and len(layers) == 2
    if name.startswith("runs_"):
        runs = (R != 0).sum(0)
        assert c.B > 256 and [int(runs[i]) for i in (5, 6, 7, 36)] == [300, 256, 257, 256]
        assert c.I - 1 == 36 and runs[36] > 0                                   # the last run of the sorted entries
        assert sorted(np.nonzero(lens == 0)[0]) == [3, c.B - 1]
        rows36 = np.nonzero(R[:, 36])[0]
        assert rows36[0] < 8 and rows36[-1] > c.B - 8                           # spread over the batch
        for item in (5, 6, 7, 36):                                              # zero coefficients inside the long runs
            bits = c.keep[np.nonzero(R.reshape(-1))[0].searchsorted(np.nonzero(R[:, item])[0] * c.I + item)]
            assert 0 < int(bits.sum()) < bits.size
        vals = set(np.unique(R[R != 0]))
        assert vals == ({1.0, 2.0, 3.0, 4.0, 5.0} if name == "runs_ratings" else {1.0})
    if name.startswith("rows_"):
        assert list(lens) == [256, 257, 512, 513, 3, 0]
    if name == "hot_softmax":
        z = VC.train_logits(name)
        assert z.max() > 88 and (z.max(1) > 88).all() and int((lens == 0).sum()) == 1
        bias = c.state["decoder.2.bias"]
        assert [float(bias[i]) for i in (5, 261, 517, 9, 265, 521)] == [100, -100, 95, -100, 0, 100]
        assert set(np.unique(bias)) == {-100.0, 0.0, 95.0, 100.0} and int((bias == 100).sum()) == 2
    # the history arrays give R back
    torch.manual_seed(0)
    m = VAECF(vae_config(user_num=c.B, item_num=c.I, mlp_hidden_size=list(c.hidden), latent_dim=c.lat,
                         history_item_id=torch.from_numpy(c.hist_id.copy()),
                         history_item_value=torch.from_numpy(c.hist_val.copy())))
    assert list(m.state_dict()) == list(c.state) and all(tuple(v.shape) == c.state[k].shape for k, v in m.state_dict().items())
    np.testing.assert_array_equal(m.get_user_rating_matrix(torch.arange(c.B)).cpu().numpy(), R)
    rp, col, val = ops.vae_history_csr(torch.from_numpy(c.hist_id.copy()), torch.from_numpy(c.hist_val.copy()), c.I)
    assert int(rp[-1]) == c.keep.size
    dense = np.zeros_like(R)
    dense[np.repeat(np.arange(c.B), np.diff(rp.numpy())), col.numpy()] = val.numpy()
    np.testing.assert_array_equal(dense, R)
    np.testing.assert_array_equal(np.nonzero(R.reshape(-1))[0], np.repeat(np.arange(c.B), np.diff(rp.numpy())) * c.I + col.numpy())
    # the reference's arithmetic in fp32 against the float64 oracle
    loss, grads = VC.restated_f32(name)
    lerr, gerr = VC.errors(loss, grads, name)
    print(name, "fp32 restatement: loss", lerr, "worst gradient", max(gerr.values()))
    assert np.isfinite(loss) and lerr <= 1e-5, (name, lerr)
    for k, e in gerr.items():
        assert e <= 1e-5, (name, k, e)
