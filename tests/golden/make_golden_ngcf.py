#!/usr/bin/env python
"""Golden vectors for NGCF, generated from the REAL reference (`daisy.model.NGCFRecommender.NGCF`, imported from the
reference checkout; nothing is copied).  Runs only where the reference exists; the output
tests/golden/kat_ngcf.npz is committed.

    python tests/golden/make_golden_ngcf.py

  (1) initial parameters under one seed and the state_dict key list;
  (2) step KATs through NGCF.calc_loss -> backward -> optimizer.step (:158-209): BPR/TL/CL, Adam (the model's
      default) and SGD, hidden lists [64,64,64], [32,16], [20], factors 36 / 64 / 20, with and without
      regularisers, mess_dropout = node_dropout = 0;
  (3) the restored embeddings and rank / full_rank / predict (:211-252);
  (4) ml-100k in run_examples/test.py's call order with --algo_name ngcf (ngcf.yaml, mess_dropout 0): one epoch
      over the first 12 800 triples (50 batches).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402

import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

if not hasattr(sp.dok_matrix, "_update"):     # NGCFRecommender.py:130 calls a private scipy method that
    sp.dok_matrix._update = lambda self, data: self._dict.update(data)   # scipy >= 1.13 removed (same effect)
import yaml  # noqa: E402
from daisy.model.NGCFRecommender import NGCF  # noqa: E402
import daisy.model.AbstractRecommender as ref_abs  # noqa: E402
from daisy.utils.dataset import BasicDataset, CandidatesDataset, get_dataloader  # noqa: E402
from daisy.utils.loader import Preprocessor, RawDataReader  # noqa: E402
from daisy.utils.sampler import BasicNegtiveSampler  # noqa: E402
from daisy.utils.splitter import TestSplitter  # noqa: E402
from daisy.utils.utils import build_candidates_set, get_inter_matrix, get_ur  # noqa: E402


def ng_config(**over):
    cfg = G.base_config()
    cfg.update(yaml.safe_load(open(os.path.join(G.REF, "daisy/assets/ngcf.yaml"))))
    cfg.update(over)
    return cfg


def random_graph(rng, U, I, n):
    gu, gi = rng.integers(0, U, n), rng.integers(0, I, n)
    gu[:5], gi[:5] = gu[5:10], gi[5:10]                      # duplicate interactions
    return gu.astype(np.int64), gi.astype(np.int64)


def make_model(cfg, gu, gi):
    cfg["inter_matrix"] = sp.coo_matrix((np.ones(len(gu), np.float32), (gu, gi)),
                                        shape=(cfg["user_num"], cfg["item_num"]))
    return NGCF(cfg)


def params_of(model, prefix):
    return {f"{prefix}/p/{k}": v.detach().numpy().copy() for k, v in model.state_dict().items()}


def kat_case(name, U, I, f, hidden, nedge, B, loss_type, optimizer, reg, lr, n_steps, rng):
    gu, gi = random_graph(rng, U, I, nedge)
    cfg = ng_config(user_num=U, item_num=I, factors=f, hidden_size_list=hidden, loss_type=loss_type,
                    optimizer=optimizer, reg_1=reg, reg_2=reg, lr=lr, epochs=1, early_stop=False,
                    init_method="default", mess_dropout=0.0, node_dropout=0.0)
    seed = int(rng.integers(1 << 30))
    torch.manual_seed(seed)
    model = make_model(cfg, gu, gi)
    out = {f"{name}/meta": np.array([U, I, f, B, n_steps, seed], dtype=np.int64),
           f"{name}/hidden": np.array(hidden, dtype=np.int64),
           f"{name}/hyper": np.array([lr, reg, reg], dtype=np.float64),
           f"{name}/loss_type": np.array(loss_type), f"{name}/optimizer": np.array(model.optimizer),
           f"{name}/gu": gu, f"{name}/gi": gi}
    out.update(params_of(model, f"{name}/init"))
    opt = model._build_optimizer(optimizer=model.optimizer, lr=model.lr)
    model.criterion = model._build_criterion(model.loss_type)
    us, is_, js, losses = [], [], [], []
    for _ in range(n_steps):
        u = rng.integers(0, U, size=B).astype(np.int32)
        i = rng.integers(0, I, size=B).astype(np.int32)
        j = (rng.integers(0, 2, size=B) if loss_type in ("CL", "SL") else rng.integers(0, I, size=B)).astype(np.int32)
        u[1] = u[0]; i[2] = i[0]
        if loss_type not in ("CL", "SL"):
            j[3] = i[0]
        model.zero_grad()
        loss = model.calc_loss([torch.from_numpy(x) for x in (u, i, j)])
        loss.backward()
        opt.step()
        us.append(u); is_.append(i); js.append(j)
        losses.append(float(loss.item()))
    out.update({f"{name}/u": np.stack(us), f"{name}/i": np.stack(is_), f"{name}/j": np.stack(js),
                f"{name}/loss": np.array(losses, dtype=np.float64)})
    out.update(params_of(model, f"{name}/final"))
    return out


def rank_case(rng):
    U, I, f, C, nB, topk = 40, 60, 16, 30, 10, 10
    gu, gi = random_graph(rng, U, I, 400)
    torch.manual_seed(3)
    model = make_model(ng_config(user_num=U, item_num=I, factors=f, hidden_size_list=[24, 8], topk=topk,
                                 mess_dropout=0.0, node_dropout=0.0), gu, gi)
    model.eval()
    us = rng.integers(0, U, size=nB).astype(np.int64)
    cands = rng.integers(0, I, size=(nB, C)).astype(np.int64)
    loader = get_dataloader(CandidatesDataset([[int(us[b]), cands[b]] for b in range(nB)]), batch_size=4,
                            shuffle=False, num_workers=0)
    preds = model.rank(loader)
    full = np.stack([model.full_rank(int(u)) for u in us])
    pred_pairs = np.array([model.predict(int(us[b]), int(cands[b, 0])) for b in range(nB)], dtype=np.float32)
    out = {"rank/meta": np.array([U, I, f], dtype=np.int64), "rank/hidden": np.array([24, 8], dtype=np.int64),
           "rank/gu": gu, "rank/gi": gi, "rank/us": us, "rank/cands": cands, "rank/topk": np.int64(topk),
           "rank/preds": preds.astype(np.float32), "rank/full": full.astype(np.int64), "rank/predict": pred_pairs,
           "rank/restore_user": model.restore_user_e.detach().numpy().copy(),
           "rank/restore_item": model.restore_item_e.detach().numpy().copy(),
           "rank/keys": np.array(list(model.state_dict().keys()))}
    out.update(params_of(model, "rank"))
    return out


def ml100k_case(n_samples=12800):
    cwd = os.getcwd()
    os.chdir(G.REF)
    try:
        cfg = ng_config(num_ng=1, epochs=1, early_stop=False, algo_name="ngcf", dataset="ml-100k", mess_dropout=0.0)
        G.seed_all(cfg["seed"])
        df = RawDataReader(cfg).get_data()
        pre = Preprocessor(cfg)
        df = pre.process(df)
        cfg["user_num"], cfg["item_num"] = pre.user_num, pre.item_num
        tr_idx, te_idx = TestSplitter(cfg).split(df)
        train_set, test_set = df.iloc[tr_idx, :].copy(), df.iloc[te_idx, :].copy()
        train_ur = get_ur(train_set)
        cfg["train_ur"] = train_ur
        cfg["inter_matrix"] = get_inter_matrix(train_set, cfg)                 # test.py:88-89
        model = NGCF(cfg)
        init = params_of(model, "ml/init")
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
    print("ml-100k NGCF: samples", samples.shape, "epoch losses", epoch_losses)
    out = {"ml/meta": np.array([cfg["user_num"], cfg["item_num"], cfg["factors"]], dtype=np.int64),
           "ml/hyper": np.array([cfg["lr"], cfg["reg_1"], cfg["reg_2"]], dtype=np.float64),
           "ml/batch_size": np.int64(cfg["batch_size"]), "ml/seed": np.int64(cfg["seed"]),
           "ml/train_users": train_set["user"].to_numpy().astype(np.int32),
           "ml/train_items": train_set["item"].to_numpy().astype(np.int32),
           "ml/samples": samples.astype(np.int32), "ml/rng_state_before_fit": rng_state,
           "ml/epoch_losses": epoch_losses, "ml/batch_losses": np.array(batch_losses, dtype=np.float64)}
    out.update(init)          # (the parameters after the 50 steps are left out: the file stays under 1 MiB)
    return out


def main():
    rng = np.random.default_rng(2021)
    out, names = {}, []
    for (name, U, I, f, hidden, ne, B, lt, opt, reg, lr, ns) in [
        ("ng_bpr_adam", 50, 40, 36, [64, 64, 64], 600, 64, "BPR", "default", 0.0, 0.01, 3),   # ngcf.yaml shape
        ("ng_bpr_adam_reg", 60, 50, 64, [32, 16], 500, 96, "BPR", "default", 1e-3, 0.01, 3),
        ("ng_bpr_sgd", 50, 40, 20, [20], 300, 64, "BPR", "sgd", 1e-3, 0.05, 3),
        ("ng_tl_sgd", 30, 40, 36, [32, 16], 200, 48, "TL", "sgd", 0.0, 0.05, 2),
        ("ng_cl_adam_reg", 50, 40, 20, [32, 16], 400, 64, "CL", "default", 1e-3, 0.01, 3),
    ]:
        out.update(kat_case(name, U, I, f, hidden, ne, B, lt, opt, reg, lr, ns, rng))
        names.append(name)
    out["names"] = np.array(names)
    out.update(rank_case(rng))
    out.update(ml100k_case())
    path = os.path.join(HERE, "kat_ngcf.npz")
    np.savez_compressed(path, **out)
    print("kat_ngcf.npz:", names, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
