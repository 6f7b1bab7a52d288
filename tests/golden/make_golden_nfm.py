#!/usr/bin/env python
"""Golden vectors for NFM, generated from the REAL reference (`daisy.model.NFMRecommender.NFM`, imported from the
reference checkout; nothing is copied).  Runs only where the reference exists; the output tests/golden/kat_nfm.npz
is committed.

    python tests/golden/make_golden_nfm.py

  (1) initial parameters / buffers under one seed and the state_dict keys for num_layers 0..3 x batch_norm on/off x
      act relu / sigmoid / tanh / other;
  (2) step KATs through NFM.calc_loss -> backward -> optimizer.step (:125-151): BPR / HL / TL / CL / SL, SGD and
      Adam, batch_norm on / off, with and without regularisers, factors 30 / 64 / 7, no dropout (NO_DROP).  Each
      stores the seed, the losses, the parameters and BatchNorm buffers after the steps;
  (3) rank / full_rank lists in eval and in training mode, predict values (batch_norm off);
  (4) ml-100k in run_examples/test.py's call order with nfm.yaml (no dropout): the losses of the first 50 batches
      of one epoch and the parameters after them.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402

import torch  # noqa: E402
import yaml  # noqa: E402
from daisy.model.NFMRecommender import NFM  # noqa: E402
import daisy.model.AbstractRecommender as ref_abs  # noqa: E402
from daisy.utils.dataset import BasicDataset, CandidatesDataset, get_dataloader  # noqa: E402
from daisy.utils.loader import Preprocessor, RawDataReader  # noqa: E402
from daisy.utils.sampler import BasicNegtiveSampler  # noqa: E402
from daisy.utils.splitter import TestSplitter  # noqa: E402
from daisy.utils.utils import get_ur  # noqa: E402


# dropout 0 cannot be recorded through autograd: nn.Dropout(p=0) hands its input back, and the in-place `fm += ...` of
# forward (:120) then modifies the saved output of the activation ("modified by an inplace operation").  A keep
# probability this close to 1 drops no element and its scale 1 / (1 - p) rounds to 1.0 in fp32: the run is the
# dropout-free one.  (The mirror's threshold for such p is 0: dropout off.)
NO_DROP = 1e-12


def nfm_config(**over):
    cfg = G.base_config()
    cfg.update(yaml.safe_load(open(os.path.join(G.REF, "daisy/assets/nfm.yaml"))))
    cfg.update(over)
    return cfg


def state_of(model, prefix):
    return {f"{prefix}/p/{k}": v.detach().numpy().copy() for k, v in model.state_dict().items()}


def init_cases():
    out, names = {}, []
    for L in (0, 1, 2, 3):
        for bn in (True, False):
            for act in ("relu", "sigmoid", "tanh", "elu"):
                name = f"init_L{L}_bn{int(bn)}_{act}"
                torch.manual_seed(100 + L)
                model = NFM(nfm_config(user_num=7, item_num=9, factors=5, num_layers=L, batch_norm=bn, act_function=act,
                                       dropout=NO_DROP))
                out.update(state_of(model, name))
                out[f"{name}/keys"] = np.array(list(model.state_dict().keys()))
                out[f"{name}/meta"] = np.array([7, 9, 5, L, int(bn), 100 + L], dtype=np.int64)
                out[f"{name}/act"] = np.array(act)
                names.append(name)
    out["init_names"] = np.array(names)
    return out


def kat_case(name, U, I, f, L, bn, act, B, loss_type, optimizer, reg, lr, n_steps, rng):
    cfg = nfm_config(user_num=U, item_num=I, factors=f, num_layers=L, batch_norm=bn, act_function=act, dropout=NO_DROP,
                     loss_type=loss_type, optimizer=optimizer, reg_1=reg, reg_2=reg, lr=lr, epochs=1, early_stop=False)
    seed = int(rng.integers(1 << 30))
    torch.manual_seed(seed)
    model = NFM(cfg)
    out = {f"{name}/meta": np.array([U, I, f, L, int(bn), B, n_steps, seed], dtype=np.int64),
           f"{name}/hyper": np.array([lr, reg, reg], dtype=np.float64), f"{name}/act": np.array(act),
           f"{name}/loss_type": np.array(loss_type), f"{name}/optimizer": np.array(model.optimizer)}
    # (the initial state is not stored: NFM(cfg) after torch.manual_seed(seed) rebuilds it - the init cases pin that)
    opt = model._build_optimizer(optimizer=model.optimizer, lr=model.lr)
    model.criterion = model._build_criterion(model.loss_type)
    model.train()
    us, is_, js, losses = [], [], [], []
    for _ in range(n_steps):
        u = rng.integers(0, U, size=B).astype(np.int32)
        i = rng.integers(0, I, size=B).astype(np.int32)
        j = (rng.integers(0, 2, size=B) if loss_type in ("CL", "SL") else rng.integers(0, I, size=B)).astype(np.int32)
        u[1] = u[0]; i[2] = i[0]
        if loss_type not in ("CL", "SL"):
            j[3] = i[0]
        model.zero_grad()
        loss = model.calc_loss([torch.from_numpy(x).long() for x in (u, i, j)])
        loss.backward()
        opt.step()
        us.append(u); is_.append(i); js.append(j)
        losses.append(float(loss.item()))
    out.update({f"{name}/u": np.stack(us), f"{name}/i": np.stack(is_), f"{name}/j": np.stack(js),
                f"{name}/loss": np.array(losses, dtype=np.float64)})
    out.update(state_of(model, f"{name}/final"))
    return out


def rank_case(rng):
    U, I, f, C, nB, topk = 40, 60, 16, 30, 10, 10
    out = {"rank/meta": np.array([U, I, f, C, nB, topk], dtype=np.int64)}
    us = rng.integers(0, U, size=nB).astype(np.int64)
    cands = rng.integers(0, I, size=(nB, C)).astype(np.int64)
    out["rank/us"], out["rank/cands"] = us, cands
    for bn in (True, False):
        for mode in ("eval", "train"):
            key = f"rank/bn{int(bn)}_{mode}"
            torch.manual_seed(3)
            model = NFM(nfm_config(user_num=U, item_num=I, factors=f, num_layers=2, batch_norm=bn, dropout=NO_DROP, topk=topk))
            with torch.no_grad():                      # non-trivial biases and running statistics
                for p in (model.u_bias.weight, model.i_bias.weight):
                    p.copy_(0.1 * torch.randn_like(p))
                for m in model.modules():
                    if isinstance(m, torch.nn.BatchNorm1d):
                        m.running_mean.copy_(0.01 * torch.randn_like(m.running_mean))
                        m.running_var.copy_(0.5 + torch.rand_like(m.running_var))
                        m.weight.copy_(1 + 0.2 * torch.randn_like(m.weight))
                        m.bias.copy_(0.1 * torch.randn_like(m.bias))
            out.update(state_of(model, f"{key}/before"))
            model.train(mode == "train")
            loader = get_dataloader(CandidatesDataset([[int(us[b]), cands[b]] for b in range(nB)]), batch_size=4,
                                    shuffle=False, num_workers=0)
            with torch.no_grad():
                out[f"{key}/preds"] = model.rank(loader).astype(np.float32)
                out[f"{key}/full"] = np.stack([model.full_rank(int(u)) for u in us]).astype(np.int64)
                if not bn:
                    out[f"{key}/predict"] = np.array([model.predict(int(us[b]), int(cands[b, 0])) for b in range(nB)],
                                                     dtype=np.float32)
            out.update(state_of(model, f"{key}/after"))
    return out


def ml100k_case(n_samples=12800):
    cwd = os.getcwd()
    os.chdir(G.REF)
    try:
        cfg = nfm_config(epochs=1, early_stop=False, algo_name="nfm", dataset="ml-100k", dropout=NO_DROP)
        G.seed_all(cfg["seed"])
        df = RawDataReader(cfg).get_data()
        pre = Preprocessor(cfg)
        df = pre.process(df)
        cfg["user_num"], cfg["item_num"] = pre.user_num, pre.item_num
        tr_idx, te_idx = TestSplitter(cfg).split(df)
        train_set = df.iloc[tr_idx, :].copy()
        cfg["train_ur"] = get_ur(train_set)
        rng_model = torch.get_rng_state().numpy().copy()      # NFM(cfg) from this state rebuilds the initial one
        model = NFM(cfg)
        samples = BasicNegtiveSampler(train_set, cfg).sampling()[:n_samples]
        loader = get_dataloader(BasicDataset(samples), batch_size=cfg["batch_size"], shuffle=True, num_workers=0)
        rng_state = torch.get_rng_state().numpy().copy()
        ref_abs.tqdm = G._TqdmCapture
        G._TqdmCapture.epoch_losses = []
        batch_losses = []
        orig = model.calc_loss

        def spy(batch):
            loss = orig(batch)
            batch_losses.append(float(loss.item()))
            return loss
        model.calc_loss = spy
        model.fit(loader)
        epoch_losses = np.array(G._TqdmCapture.epoch_losses, dtype=np.float64)
    finally:
        os.chdir(cwd)
    print("ml-100k NFM: samples", samples.shape, "epoch losses", epoch_losses)
    out = {"ml/meta": np.array([cfg["user_num"], cfg["item_num"], cfg["factors"], cfg["num_layers"]], dtype=np.int64),
           "ml/hyper": np.array([cfg["lr"], cfg["reg_1"], cfg["reg_2"]], dtype=np.float64),
           "ml/batch_size": np.int64(cfg["batch_size"]), "ml/seed": np.int64(cfg["seed"]),
           "ml/samples": samples.astype(np.int32), "ml/rng_state_before_fit": rng_state,
           "ml/rng_state_before_model": rng_model,
           "ml/epoch_losses": epoch_losses, "ml/batch_losses": np.array(batch_losses, dtype=np.float64)}
    out.update(state_of(model, "ml/final"))
    return out


def main():
    rng = np.random.default_rng(2024)
    out, names = {}, []
    out.update(init_cases())
    for (name, U, I, f, L, bn, act, B, lt, opt, reg, lr, ns) in [
        ("nf_bpr_sgd", 50, 40, 30, 2, True, "relu", 64, "BPR", "default", 0.0, 0.05, 3),       # nfm.yaml shape
        ("nf_bpr_sgd_nobn", 50, 40, 30, 2, False, "relu", 64, "BPR", "default", 0.0, 0.05, 3),
        ("nf_bpr_adam_reg", 60, 50, 64, 2, True, "relu", 96, "BPR", "adam", 1e-3, 0.01, 3),
        ("nf_hl_sgd_reg", 50, 40, 7, 1, True, "tanh", 48, "HL", "sgd", 1e-3, 0.05, 2),
        ("nf_tl_adam", 30, 40, 30, 3, True, "sigmoid", 48, "TL", "adam", 0.0, 0.01, 2),
        ("nf_cl_sgd_reg", 50, 40, 7, 2, False, "sigmoid", 64, "CL", "sgd", 1e-3, 0.05, 3),
        ("nf_cl_adam", 50, 40, 30, 1, True, "relu", 64, "CL", "adam", 0.0, 0.01, 2),
        ("nf_sl_sgd", 40, 30, 64, 0, True, "relu", 32, "SL", "sgd", 0.0, 0.01, 2),
        ("nf_sl_adam_reg_nobn", 40, 30, 30, 2, False, "tanh", 32, "SL", "adam", 1e-3, 0.01, 2),
        ("nf_bpr_adam_L0_nobn", 40, 30, 7, 0, False, "relu", 32, "BPR", "adam", 1e-3, 0.01, 2),
        ("nf_hl_adam_other", 40, 30, 30, 2, True, "elu", 32, "HL", "adam", 0.0, 0.01, 2),
    ]:
        out.update(kat_case(name, U, I, f, L, bn, act, B, lt, opt, reg, lr, ns, rng))
        names.append(name)
    out["names"] = np.array(names)
    out.update(rank_case(rng))
    out.update(ml100k_case())
    path = os.path.join(HERE, "kat_nfm.npz")
    np.savez_compressed(path, **out)
    print("kat_nfm.npz:", names, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
