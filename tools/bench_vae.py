#!/usr/bin/env python
"""Multi-VAE step and scoring rates on one device.  Histories are seeded synthetic data with Zipf item
popularity.

    python tools/bench_vae.py [--out profiles/bench_vae.json] [--steps 20]

Per shape: the HIP step (daisy_vae_fit_epoch: forward, backward, dense Adam) in µs against stock torch on the same device
(autograd over the reference's module structure, the dense B x I rating rows, torch.optim.Adam), and for the large
catalogue the floor: fp32 GEMM FLOPs / 155 TF/s plus the dense Adam's bytes / the device copy rate measured here.
Then rank (1 000 candidates x 256 users) and full_rank rates.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from daisyrec_amd import ops  # noqa: E402

FP32_MFMA_TFLOPS = 155.0


def histories(U, I, mean_len, seed, zipf=1.0):
    """CSR of seeded histories: lengths ~ 1 + geometric(mean_len); items drawn with Zipf popularity
    (p_i ~ 1 / (rank_i + 1)^zipf over a seeded permutation of the ids, the repeats of a row dropped), so popular items
    sit in a large share of the rows as in the real data sets"""
    rng = np.random.default_rng(seed)
    lens = np.minimum(1 + rng.geometric(1.0 / mean_len, size=U), I)
    cdf = np.cumsum(1.0 / np.arange(1, I + 1) ** zipf)
    cdf /= cdf[-1]
    ids = rng.permutation(I)
    cols = [np.unique(ids[np.minimum(np.searchsorted(cdf, rng.random(int(n))), I - 1)]) for n in lens]
    lens = np.array([c.size for c in cols], dtype=np.int64)
    row_ptr = np.zeros(U + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum(lens)
    col = np.concatenate(cols).astype(np.int32)
    dev = "cuda"
    top = np.bincount(col, minlength=I).max()
    return (torch.from_numpy(row_ptr).to(dev), torch.from_numpy(col).to(dev), torch.ones(col.size, device=dev)), lens, top


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def flat_params(I, hidden, lat, seed):
    """the flat buffer of daisy_vae_* (encoder.0.weight item-major) from an initialised torch module of the same shape"""
    torch.manual_seed(seed)
    enc = [I] + hidden + [lat]
    dec = [lat // 2] + hidden[::-1] + [I]
    parts = []
    for dims, first in ((enc, True), (dec, False)):
        for k, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
            w = torch.empty(b, a)
            nn.init.xavier_normal_(w)
            parts.append((w.t() if (first and k == 0) else w).reshape(-1))
            parts.append(torch.zeros(b))
    return torch.cat(parts).cuda()


class TorchVAE(nn.Module):
    """the reference's module structure and loss in stock torch (autograd)"""

    def __init__(self, I, hidden, lat):
        super().__init__()
        dims = [I] + hidden + [lat]
        ddims = [lat // 2] + hidden[::-1] + [I]
        mk = lambda d: nn.Sequential(*sum([[nn.Linear(a, b)] + ([nn.Tanh()] if k < len(d) - 2 else [])   # noqa: E731
                                            for k, (a, b) in enumerate(zip(d[:-1], d[1:]))], []))
        self.encoder, self.decoder, self.lat = mk(dims), mk(ddims), lat

    def loss(self, R, p=0.5, anneal=0.2):
        h = F.dropout(F.normalize(R), p, training=True)
        h = self.encoder(h)
        mu, logvar = h[:, :self.lat // 2], h[:, (self.lat + 1) // 2:]
        z = self.decoder(torch.randn_like(mu) * torch.exp(0.5 * logvar) + mu)
        kl = -0.5 * torch.mean(torch.sum(1 + logvar - mu.pow(2) - logvar.exp(), dim=1)) * anneal
        return -(F.log_softmax(z, 1) * R).sum(1).mean() + kl


def bench_shape(name, U, I, B, mean_len, steps, warmup, hidden=(600,), lat=128, torch_baseline=True, floor=False):
    hidden = list(hidden)
    csr, lens, top = histories(U, I, mean_len, seed=U ^ I)
    rng = np.random.default_rng(7)
    nb = steps + warmup
    order = np.concatenate([rng.permutation(U) for _ in range((nb * B) // U + 1)])[:nb * B]
    ent = [int(lens[order[k * B:(k + 1) * B]].sum()) for k in range(nb)]
    W = flat_params(I, hidden, lat, 0)
    g = torch.zeros_like(W)
    ctx = ops.VaeContext(B, max(ent), I, hidden, lat)
    assert ctx.param_count == W.numel()
    optim = ops.DenseOptimizer("adam", 1e-3)
    users = torch.from_numpy(order.astype(np.int64)).cuda()
    # warm-up batches, then the timed ones in ONE library call (the product path of VAECF.fit)
    ctx.fit_epoch(W, g, csr, users[:warmup * B], B, ent[:warmup], optim, 0.5, 0.2, 100000, 0, seed_hi=1 << 32)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctx.fit_epoch(W, g, csr, users[warmup * B:], B, ent[warmup:], optim, 0.5, 0.2, 100000, warmup, seed_hi=1 << 32,
                  step0=warmup)
    torch.cuda.synchronize()
    hip_us = (time.perf_counter() - t0) / steps * 1e6
    res = {"shape": name, "U": U, "I": I, "B": B, "hidden": hidden, "lat": lat, "mean_history": round(float(lens.mean()), 1),
           "top_item_share": round(float(top) / U, 3),
           "hip_step_us": round(hip_us, 1), "params": int(W.numel()), "ctx_MB": round(ctx.nbytes / 2 ** 20, 1)}
    ctx.close()
    if torch_baseline:
        model = TorchVAE(I, hidden, lat).cuda()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        rp, col, _ = (t.cpu() for t in csr)
        # the dense rating rows are built on the host outside the timing: time the device work only
        Rs = []
        for k in range(min(nb, 8)):
            us = order[k * B:(k + 1) * B]
            R = torch.zeros(B, I)
            for r, u in enumerate(us):
                R[r, col[rp[u]:rp[u + 1]].long()] = 1.0
            Rs.append(R.cuda())
        j = iter(range(10 ** 9))

        def dstep():
            R = Rs[next(j) % len(Rs)]
            opt.zero_grad()
            model.loss(R).backward()
            opt.step()
        t = timed(dstep, steps, warmup)
        res["torch_step_us"] = round(t * 1e6, 1)
        res["speedup_vs_torch"] = round(t * 1e6 / hip_us, 2)
    if floor:
        flops = 6.0 * B * I * hidden[0]
        for a, b in zip(([I] + hidden + [lat])[1:-1], ([I] + hidden + [lat])[2:]):
            flops += 6.0 * B * a * b
        flops += 6.0 * B * (lat // 2) * hidden[-1]
        x = torch.empty(256 * 2 ** 20, dtype=torch.uint8, device="cuda")
        y = torch.empty_like(x)
        tc = timed(lambda: y.copy_(x), 10, 3)
        copy_rate = 2 * x.numel() / tc                       # bytes read + written per second
        adam_bytes = 8.0 * 4 * W.numel()                     # W, g, m, v read; W, m, v, g written
        floor_us = (flops / (FP32_MFMA_TFLOPS * 1e12) + adam_bytes / copy_rate) * 1e6
        res.update(gemm_gflop=round(flops / 1e9, 1), adam_GB=round(adam_bytes / 1e9, 2),
                   copy_GBps=round(copy_rate / 1e9, 0), floor_us=round(floor_us, 1),
                   vs_floor=round(hip_us / floor_us, 2))
    return res, (csr, lens, W, hidden, lat)


def bench_rank(state, I, nU=256, C=1000, reps=10):
    csr, lens, W, hidden, lat = state
    rng = np.random.default_rng(3)
    users = torch.from_numpy(rng.choice(len(lens), size=nU, replace=False).astype(np.int64))
    E = int(lens[users.numpy()].sum())
    ctx = ops.VaeContext(nU, E, I, hidden, lat)
    cands = torch.from_numpy(rng.integers(0, I, size=(nU, C))).cuda()
    ud = users.cuda()
    t = timed(lambda: ops.topk_from_scores(ctx.scores(W, csr, ud, E, items=cands), cands, 50), reps, 2)
    u1 = users[:1].cuda()
    e1 = int(lens[users[:1].numpy()].sum())
    tf = timed(lambda: ops.full_topk_from_scores(ctx.scores(W, csr, u1, e1).view(-1), 50), reps, 2)
    ctx.close()
    return {"rank_users_per_s": round(nU / t, 0), "rank_ms_per_256x1000": round(t * 1e3, 3),
            "full_rank_users_per_s": round(1.0 / tf, 0)}


SHAPES = {
    "ml-100k": ("ml-100k (multi-vae.yaml)", 943, 1682, 256, 106),
    "ml-1m": ("ml-1m B=256", 6040, 3706, 256, 165),
    "ml-1m-2048": ("ml-1m B=2048", 6040, 3706, 2048, 165),
    "amazon": ("Amazon-Book", 52643, 91599, 256, 45),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "bench_vae.json"))
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append",
                    help="the shapes to run (default: all); e.g. for a kernel trace of one of them")
    ap.add_argument("--no-torch", action="store_true", help="skip the stock-torch baseline")
    a = ap.parse_args()
    rows = []
    for key in (a.shape or list(SHAPES)):
        name, U, I, B, mean_len = SHAPES[key]
        r, st = bench_shape(name, U, I, B, mean_len, a.steps, a.warmup, torch_baseline=not a.no_torch,
                            floor=(key == "amazon"))
        if key in ("ml-100k", "amazon"):
            r.update(bench_rank(st, I))
        rows.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "histories": "Zipf(1.0) item popularity", "rows": rows},
                      fh, indent=1)


if __name__ == "__main__":
    main()
