#!/usr/bin/env python
"""NFM measurements, one JSON line per leg:
  (a) the library's epoch loop (daisy_nfm_fit_epoch) at nfm.yaml defaults on ml-100k-sized tables, B = 256:
      us per step on the layered path (the default) and on the forced one-workgroup small path (dispatches per step:
      from a rocprofv3 kernel trace of this tool, --steps small);
  (b) a stock-torch restatement of the reference formulation (autograd, nn.BatchNorm1d, torch.optim.SGD) at the same
      shapes on the same GPU;
  (c) the step at ml-1m-like shapes, factors 64, L = 2, B = 65 536: samples/s, algorithmic bytes over kernel time
      against the device-copy rate measured in this process;
  (d) eval scoring: full_rank over 100 K items and rank over 1 000 candidates x 256 users, bytes over time against
      the copy rate.

    python tools/bench_nfm.py [--steps 200]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from daisyrec_amd import ops  # noqa: E402
from daisyrec_amd.model import NFM  # noqa: E402


def config(U, I, d, L, **over):
    import logging
    cfg = dict(gpu="0", seed=2022, topk=50, batch_size=256, loss_type="BPR", init_method="default", optimizer="default",
               early_stop=False, factors=d, act_function="relu", num_layers=L, batch_norm=True, dropout=0.5, epochs=1,
               lr=1e-3, reg_1=0.0, reg_2=0.0, user_num=U, item_num=I, logger=logging.getLogger("bench"), progress=False)
    cfg.update(over)
    return cfg


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3          # us per call


def copy_rate():
    x = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    y = torch.empty_like(x)
    us = timed(lambda: y.copy_(x), 20)
    return 2 * x.numel() * 4 / (us * 1e-6)


def library_epoch(U, I, d, L, B, steps, dropout=0.5, path="auto"):
    torch.manual_seed(0)
    m = NFM(config(U, I, d, L, dropout=dropout, step_path=path))
    p = m._params()
    n = B * steps
    g = torch.Generator(device="cuda").manual_seed(1)
    u = torch.randint(0, U, (n,), device="cuda", dtype=torch.int32, generator=g)
    i = torch.randint(0, I, (n,), device="cuda", dtype=torch.int32, generator=g)
    j = torch.randint(0, I, (n,), device="cuda", dtype=torch.int32, generator=g)
    gflat = torch.zeros_like(m._flat)
    grads = m._grad_table(gflat)
    optim = ops.DenseOptimizer("sgd", m.lr)
    ctx = m._ctx(B)

    def epoch():
        optim.t = 0
        ctx.fit_epoch(p, grads, m._bn(), u, i, j, B, optim, m._flat, gflat, ops.LOSS_IDS["BPR"], dropout=dropout,
                      seed_hi=1 << 32, step0=0)
    us = timed(epoch, 3) / steps
    ctx.close()
    return us


class TorchNFM(nn.Module):
    """the reference's formulation (NFMRecommender.py:110-151) in stock torch"""

    def __init__(self, U, I, d, L, p):
        super().__init__()
        self.P, self.Q = nn.Embedding(U, d), nn.Embedding(I, d)
        self.ub, self.ib = nn.Embedding(U, 1), nn.Embedding(I, 1)
        self.bias_ = nn.Parameter(torch.zeros(1))
        self.fm = nn.Sequential(nn.BatchNorm1d(d), nn.Dropout(p))
        mods = []
        for _ in range(L):
            mods += [nn.Linear(d, d), nn.BatchNorm1d(d), nn.ReLU(), nn.Dropout(p)]
        self.deep = nn.Sequential(*mods)
        self.pred = nn.Linear(d, 1, bias=False)

    def forward(self, u, i):
        h = self.deep(self.fm(self.P(u) * self.Q(i)))
        h = h + self.ub(u) + self.ib(i) + self.bias_
        return self.pred(h).view(-1)


def torch_step_us(U, I, d, L, B, steps):
    torch.manual_seed(0)
    m = TorchNFM(U, I, d, L, 0.5).cuda()
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    u = torch.randint(0, U, (B,), device="cuda")
    i = torch.randint(0, I, (B,), device="cuda")
    j = torch.randint(0, I, (B,), device="cuda")

    def step():
        opt.zero_grad()
        loss = -(1e-10 + torch.sigmoid(m(u, i) - m(u, j))).log().sum()
        loss.backward()
        opt.step()
    return timed(step, steps)


def step_bytes(R, d, L):
    """algorithmic bytes of one step over R rows: the two embedding gathers, every stage's activations written once
    and read once by the backward pass, the gradient of every stage written and read once, the embedding gradient
    rows written once (fp32)"""
    return 4 * R * d * (2 + 2 * (L + 1) + 2 * (L + 1) + 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--only", choices=["a", "c"], help="run one leg of the library alone (for a kernel trace)")
    a = ap.parse_args()
    if a.only == "a":
        print(json.dumps({"a_us_per_step": library_epoch(943, 1682, 30, 2, 256, a.steps), "steps_run": 4 * a.steps}))
        return
    if a.only == "c":
        print(json.dumps({"c_us_per_step": library_epoch(6040, 3706, 64, 2, 65536, a.steps, dropout=0.0),
                          "steps_run": 4 * a.steps}))
        return
    rate = copy_rate()
    out = {"copy_GBps": rate / 1e9}
    # (a), (b): nfm.yaml defaults, ml-100k tables
    out["a_us_per_step"] = library_epoch(943, 1682, 30, 2, 256, a.steps)
    out["a_small_path_us_per_step"] = library_epoch(943, 1682, 30, 2, 256, a.steps, path="small")
    out["b_torch_us_per_step"] = torch_step_us(943, 1682, 30, 2, 256, a.steps)
    out["a_speedup_vs_b"] = out["b_torch_us_per_step"] / out["a_us_per_step"]
    # (c): ml-1m-like, d = 64, L = 2, B = 65 536 (no dropout: the layered step's arithmetic)
    us = library_epoch(6040, 3706, 64, 2, 65536, 8, dropout=0.0)
    out["c_us_per_step"] = us
    out["c_samples_per_s"] = 65536 / (us * 1e-6)
    out["c_frac_of_copy"] = step_bytes(2 * 65536, 64, 2) / (us * 1e-6) / rate
    # (d): eval scoring, d = 30, L = 2, BatchNorm with running statistics
    torch.manual_seed(0)
    m = NFM(config(256, 100000, 30, 2))
    m.eval()
    p = m._params()
    ctx = m._ctx(1)
    user = torch.tensor([3], device="cuda")
    us_full = timed(lambda: ctx.scores(p, m._bn(), user, None, C_=0, n=100000), 50)
    users = torch.arange(256, device="cuda")
    cands = torch.randint(0, 100000, (256 * 1000,), device="cuda")
    us_rank = timed(lambda: ctx.scores(p, m._bn(), users, cands, C_=1000), 50)
    ctx.close()
    out["d_full_rank_us"] = us_full
    out["d_full_rank_frac_of_copy"] = (100000 * (30 + 1) * 4 + 100000 * 4) / (us_full * 1e-6) / rate
    out["d_rank_us"] = us_rank
    out["d_rank_frac_of_copy"] = (256000 * (30 + 1) * 4 + 256000 * 8 + 256000 * 4) / (us_rank * 1e-6) / rate
    print(json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in out.items()}))


if __name__ == "__main__":
    main()
