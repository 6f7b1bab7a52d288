#!/usr/bin/env python
"""Golden vectors for Multi-VAE, generated from the REAL reference (`daisy.model.VAECFRecommender.VAECF`, imported from
the reference checkout; nothing is copied).  Runs only where the reference exists; the outputs are committed:

    python tests/golden/make_golden_vae.py        # -> tests/golden/kat_vae.npz, tests/golden/kat_vae_ml100k.npz

The reference's own noise is recorded by wrapping torch.nn.functional.dropout and torch.randn_like in this process
(the draws themselves are untouched): the keep bits of the input dropout where R != 0 (row-major, i.e. per row the
items ascending) and the reparameterisation's eps.

kat_vae.npz:
  (1) initial parameters and state_dict keys under one seed: the default shape, an odd latent_dim, two hidden layers;
  (2) step KATs through VAECF.calc_loss -> backward -> optimizer.step (Adam / SGD / Adagrad / RMSprop) on small
      catalogues: a user with item 0 in a history shorter than the longest (erased) and one in the longest (kept), a
      row that is empty after that rule, anneal below and at its cap (total_anneal_steps 3 and 0);
  (3) rank in eval and in training mode (the noise of every forward call), full_rank and predict in eval mode.
kat_vae_ml100k.npz: ml-100k in run_examples/test.py's call order with multi-vae.yaml for 2 epochs: the train split's
  histories, the loader's order, every batch's loss and noise, the epoch losses, a seeded sample of the final
  parameters and the eval-mode rank lists of test.py's first 64 candidate users.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402

import pandas as pd  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import yaml  # noqa: E402
import daisy.model.AbstractRecommender as ref_abs  # noqa: E402
from daisy.model.VAECFRecommender import VAECF  # noqa: E402
from daisy.utils.dataset import AEDataset, CandidatesDataset, get_dataloader  # noqa: E402
from daisy.utils.loader import Preprocessor, RawDataReader  # noqa: E402
from daisy.utils.splitter import TestSplitter  # noqa: E402
from daisy.utils.utils import build_candidates_set, get_history_matrix, get_ur  # noqa: E402


class NoiseRecorder:
    """Records every training-mode input dropout (keep bits where the input is non-zero) and randn_like draw."""

    def __init__(self):
        self.keep, self.eps = [], []
        self._drop, self._randn = F.dropout, torch.randn_like

    def __enter__(self):
        rec = self

        def dropout(x, p=0.5, training=True, inplace=False):
            out = rec._drop(x, p, training, inplace)
            if training and p > 0:
                rec.keep.append((out != 0)[x != 0].numpy().astype(np.uint8))
            return out

        def randn_like(t, *a, **k):
            out = rec._randn(t, *a, **k)
            rec.eps.append(out.detach().numpy().copy())
            return out
        F.dropout, torch.randn_like = dropout, randn_like
        return self

    def __exit__(self, *exc):
        F.dropout, torch.randn_like = self._drop, self._randn


def vae_config(**over):
    cfg = G.base_config()
    cfg.update(yaml.safe_load(open(os.path.join(G.REF, "daisy/assets/multi-vae.yaml"))))
    cfg.update(algo_name="multi-vae")
    cfg.update(over)
    return cfg


def history(pairs, U, I):
    """get_history_matrix of the reference over (user, item) rows in the given order"""
    df = pd.DataFrame({"user": [p[0] for p in pairs], "item": [p[1] for p in pairs], "rating": 1.0})
    cfg = vae_config(user_num=U, item_num=I)
    hid, hval, _ = get_history_matrix(df, cfg, row="user")
    return hid, hval


def state_of(model, prefix):
    return {f"{prefix}/p/{k}": v.detach().numpy().copy() for k, v in model.state_dict().items()}


def init_cases():
    out, names = {}, []
    hid, hval = history([(0, 1), (1, 2)], 3, 11)
    for name, hidden, lat in (("init_default", None, 128), ("init_odd_lat", [9], 7), ("init_two_hidden", [12, 10], 6)):
        torch.manual_seed(7)
        m = VAECF(vae_config(user_num=3, item_num=11, mlp_hidden_size=hidden, latent_dim=lat, history_item_id=hid,
                             history_item_value=hval))
        if hidden is None:             # the default shape is large: its tensors as digests (bitwise equality is the test)
            import hashlib
            for k, v in m.state_dict().items():
                out[f"{name}/sha/{k}"] = np.array(hashlib.sha256(v.numpy().tobytes()).hexdigest())
                out[f"{name}/shape/{k}"] = np.array(v.shape, dtype=np.int64)
        else:
            out.update(state_of(m, name))
        out[f"{name}/keys"] = np.array(list(m.state_dict().keys()))
        out[f"{name}/meta"] = np.array([3, 11, lat, 7], dtype=np.int64)
        out[f"{name}/hidden"] = np.array(hidden if hidden is not None else [], dtype=np.int64)
        names.append(name)
    out["init_names"] = np.array(names)
    out["init_hist_id"], out["init_hist_val"] = hid.numpy(), hval.numpy()
    return out


def kat_histories(rng, U, I):
    """random histories (items distinct per user) with the hard cases of the item-0 rule"""
    pairs = []
    L = 9
    for u in range(U):
        n = int(rng.integers(1, L))
        items = [int(x) for x in rng.choice(np.arange(1, I), size=n, replace=False)]
        if u == 1:
            items = [0] + items[:3]                   # item 0 in a short row: erased
        if u == 2:
            items = [0]                               # only item 0, short row: the row is empty
        if u == 3:
            items = [0] + [int(x) for x in rng.choice(np.arange(1, I), size=L - 1, replace=False)]   # the longest row
        pairs += [(u, i) for i in items]
    order = rng.permutation(len(pairs))
    return [pairs[k] for k in order]


def kat_case(name, rng, optimizer, hidden, lat, total_anneal, lr, n_steps=2, U=10, I=24, B=6):
    hid, hval = history(kat_histories(rng, U, I), U, I)
    seed = int(rng.integers(1 << 30))
    cfg = vae_config(user_num=U, item_num=I, mlp_hidden_size=hidden, latent_dim=lat, history_item_id=hid,
                     history_item_value=hval, optimizer=optimizer, lr=lr, total_anneal_steps=total_anneal, epochs=1,
                     early_stop=False)
    torch.manual_seed(seed)
    model = VAECF(cfg)
    out = {f"{name}/meta": np.array([U, I, lat, B, n_steps, seed, total_anneal], dtype=np.int64),
           f"{name}/hidden": np.array(hidden if hidden is not None else [], dtype=np.int64),
           f"{name}/hyper": np.array([lr, cfg["dropout"], cfg["anneal_cap"]], dtype=np.float64),
           f"{name}/optimizer": np.array(model.optimizer), f"{name}/hist_id": hid.numpy(),
           f"{name}/hist_val": hval.numpy()}
    opt = model._build_optimizer(optimizer=model.optimizer, lr=model.lr)
    model.train()
    users, losses, Rs = [], [], []
    for k in range(n_steps):
        us = rng.choice(U, size=B, replace=False)
        if k == 0:
            us[:4] = [1, 2, 3, 0]
        u = torch.from_numpy(us.astype(np.int64))
        Rs.append(model.get_user_rating_matrix(u).numpy())
        with NoiseRecorder() as rec:
            model.zero_grad()
            loss = model.calc_loss(u)
        loss.backward()
        opt.step()
        assert len(rec.keep) == 1 and len(rec.eps) == 1
        out[f"{name}/keep{k}"] = rec.keep[0]
        out[f"{name}/eps{k}"] = rec.eps[0]
        users.append(us)
        losses.append(float(loss.item()))
    out.update({f"{name}/users": np.stack(users).astype(np.int64), f"{name}/loss": np.array(losses, dtype=np.float64),
                f"{name}/R": np.stack(Rs), f"{name}/update": np.int64(model.update)})
    out.update(state_of(model, f"{name}/final"))
    return out


def rank_case(rng):
    U, I, C, nB, topk, lat = 30, 50, 20, 10, 10, 8
    hid, hval = history(kat_histories(rng, U, I), U, I)
    out = {"rank/meta": np.array([U, I, C, nB, topk, lat, 3], dtype=np.int64), "rank/hist_id": hid.numpy(),
           "rank/hist_val": hval.numpy()}
    us = rng.choice(U, size=nB, replace=False).astype(np.int64)
    cands = rng.integers(0, I, size=(nB, C)).astype(np.int64)
    out["rank/us"], out["rank/cands"] = us, cands
    for mode in ("eval", "train"):
        key = f"rank/{mode}"
        torch.manual_seed(3)
        model = VAECF(vae_config(user_num=U, item_num=I, mlp_hidden_size=[16], latent_dim=lat, history_item_id=hid,
                                 history_item_value=hval, topk=topk))
        with torch.no_grad():                         # non-trivial biases
            for m in model.modules():
                if isinstance(m, torch.nn.Linear):
                    m.bias.copy_(0.1 * torch.randn_like(m.bias))
        if mode == "eval":
            out.update(state_of(model, "rank/params"))
        model.train(mode == "train")
        loader = get_dataloader(CandidatesDataset([[int(us[b]), cands[b]] for b in range(nB)]), batch_size=4,
                                shuffle=False, num_workers=0)
        with torch.no_grad(), NoiseRecorder() as rec:
            out[f"{key}/preds"] = model.rank(loader).astype(np.float32)
            if mode == "eval":
                out[f"{key}/full"] = np.stack([model.full_rank(int(u)) for u in us]).astype(np.int64)
                out[f"{key}/predict"] = np.array([model.predict(int(us[b]), int(cands[b, 0])) for b in range(nB)],
                                                 dtype=np.float32)
        if mode == "train":
            assert len(rec.keep) == 3 and len(rec.eps) == 3
            for k in range(3):
                out[f"{key}/keep{k}"], out[f"{key}/eps{k}"] = rec.keep[k], rec.eps[k]
    return out


def ml100k_case():
    cwd = os.getcwd()
    os.chdir(G.REF)
    try:
        cfg = vae_config(epochs=2, early_stop=False, dataset="ml-100k")
        G.seed_all(cfg["seed"])
        df = RawDataReader(cfg).get_data()
        pre = Preprocessor(cfg)
        df = pre.process(df)
        cfg["user_num"], cfg["item_num"] = pre.user_num, pre.item_num
        tr_idx, te_idx = TestSplitter(cfg).split(df)
        train_set, test_set = df.iloc[tr_idx, :].copy(), df.iloc[te_idx, :].copy()
        test_ur = get_ur(test_set)
        total_train_ur = get_ur(train_set)
        cfg["train_ur"] = total_train_ur
        hid, hval, hlen = get_history_matrix(train_set, cfg, row="user")
        cfg["history_item_id"], cfg["history_item_value"] = hid, hval
        rng_model = torch.get_rng_state().numpy().copy()      # VAECF(cfg) from this state rebuilds the initial one
        model = VAECF(cfg)
        ds = AEDataset(train_set, yield_col=cfg["UID_NAME"])
        loader = get_dataloader(ds, batch_size=cfg["batch_size"], shuffle=True, num_workers=0)
        ref_abs.tqdm = G._TqdmCapture
        G._TqdmCapture.epoch_losses = []
        batch_users, batch_losses = [], []
        orig = model.calc_loss

        def spy(batch):
            batch_users.append(batch.numpy().astype(np.int64).copy())
            loss = orig(batch)
            batch_losses.append(float(loss.item()))
            return loss
        model.calc_loss = spy
        with NoiseRecorder() as rec:
            model.fit(loader)
        epoch_losses = np.array(G._TqdmCapture.epoch_losses, dtype=np.float64)
        # test.py:112-120 - the eval-mode rank lists of the first 64 candidate users
        test_u, test_ucands = build_candidates_set(test_ur, total_train_ur, cfg)
        nU = 64
        loader_t = get_dataloader(CandidatesDataset(test_ucands[:nU]), batch_size=nU, shuffle=False, num_workers=0)
        preds = model.rank(loader_t)
    finally:
        os.chdir(cwd)
    print("ml-100k multi-vae: epoch losses", epoch_losses, "batches", len(batch_losses))
    lens = hlen.numpy()
    out = {"ml/meta": np.array([cfg["user_num"], cfg["item_num"], cfg["latent_dim"], cfg["batch_size"], cfg["seed"],
                                cfg["total_anneal_steps"]], dtype=np.int64),
           "ml/hyper": np.array([cfg["lr"], cfg["dropout"], cfg["anneal_cap"]], dtype=np.float64),
           "ml/hist_len": lens.astype(np.int32),
           "ml/hist_items": np.concatenate([hid.numpy()[u, :lens[u]] for u in range(len(lens))]).astype(np.int16),
           "ml/rng_state_before_model": rng_model, "ml/epoch_losses": epoch_losses,
           "ml/batch_losses": np.array(batch_losses, dtype=np.float64), "ml/n_batches": np.int64(len(batch_users)),
           "ml/update": np.int64(model.update)}
    for k, (us, kp, ep) in enumerate(zip(batch_users, rec.keep, rec.eps)):
        out[f"ml/users{k}"] = us
        out[f"ml/keep{k}"] = np.packbits(kp)
        out[f"ml/nkeep{k}"] = np.int64(kp.size)
        out[f"ml/eps{k}"] = ep
    # a seeded sample of the final parameters: the small tensors whole, rows / columns of the catalogue-sized ones
    srng = np.random.default_rng(5)
    for k, v in model.state_dict().items():
        v = v.numpy()
        if v.ndim == 1:
            out[f"ml/final/{k}"] = v.copy()
            continue
        axis = 1 if k == "encoder.0.weight" else 0          # (encoder.0.weight: columns = items)
        idx = np.sort(srng.choice(v.shape[axis], size=min(16, v.shape[axis]), replace=False)).astype(np.int64)
        out[f"ml/final_idx/{k}"] = idx
        out[f"ml/final/{k}"] = np.take(v, idx, axis=axis).copy()
    out["ml/rank_users"] = np.array([int(x[0]) for x in test_ucands[:nU]], dtype=np.int64)
    out["ml/rank_cands"] = np.stack([np.asarray(x[1]) for x in test_ucands[:nU]]).astype(np.int16)
    out["ml/rank_preds"] = preds.astype(np.int16)
    return out


def main():
    rng = np.random.default_rng(2026)
    out, names = {}, []
    out.update(init_cases())
    for (name, opt, hidden, lat, total, lr) in [
        ("vae_adam", "default", [16], 8, 100000, 1e-3),
        ("vae_sgd", "sgd", [16], 8, 3, 0.05),
        ("vae_adagrad", "adagrad", [12, 10], 6, 0, 0.01),
        ("vae_rmsprop_odd", "rmsprop", [16], 7, 3, 1e-3),
    ]:
        out.update(kat_case(name, rng, opt, hidden, lat, total, lr, n_steps=4 if total == 3 else 2))
        names.append(name)
    out["names"] = np.array(names)
    out.update(rank_case(rng))
    path = os.path.join(HERE, "kat_vae.npz")
    np.savez_compressed(path, **out)
    print("kat_vae.npz:", names, os.path.getsize(path), "bytes")
    path = os.path.join(HERE, "kat_vae_ml100k.npz")
    np.savez_compressed(path, **ml100k_case())
    print("kat_vae_ml100k.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
