#!/usr/bin/env python
"""Times the three stages of SLiM on the device (csrc/slim.hip): the Gram matrix, the coordinate descent over all columns
and one rank batch (128 users x 1000 candidates), at ml-100k's shape (943 x 1682, 100 000 ratings) and at a synthetic
ml-1m-like shape (6040 x 3706, about 1 M ratings), ratings 1..5, slim.yaml's alpha = 1.0 / elastic = 0.1 / topk = 50.
The data is generated from a seed (popularity-skewed items); nothing is read from disk.

    python tools/slim_bench.py [--sizes ml100k,ml1m] [--reps 5]         # needs a HIP device; prints text + one JSON line

Times are device events around windows of back-to-back calls of the stage (about 0.25 s each; median, minimum and maximum of
--reps windows after a warm-up call); `fit` and `rank` are host clocks
around SLiM.fit(DataFrame) / SLiM.rank(loader), which end in a device-to-host copy.  For the descent the script counts the
bytes of Gram rows its H updates read (every coordinate update that changes a value reads one row: `moves` x item_num x 4)
and the rows the sweeps themselves read (column j and the diagonal, once per sweep), and sets the rate against the
cache rates of the MI355X notes: about 34.5 TB/s for the eight L2s together, about 8.6 TB/s for rows gathered from the
Infinity Cache, about 6.3 TB/s from HBM.
"""
import argparse
import json
import statistics
import time

import numpy as np

SIZES = {"ml100k": (943, 1682, 100_000), "ml1m": (6040, 3706, 1_000_000)}
L2_TBS, MALL_TBS, HBM_TBS = 34.5, 8.6, 6.3


def synth(U, I, n, seed=0):
    rng = np.random.RandomState(seed)
    pop = rng.zipf(1.3, I).clip(1, 200).astype(float)
    key = np.unique(rng.randint(0, U, 2 * n).astype(np.int64) * I + rng.choice(I, 2 * n, p=pop / pop.sum()))
    key = rng.permutation(key)[:n]
    return key // I, key % I, rng.randint(1, 6, len(key)).astype(np.float64)


WINDOW_S = 0.25        # a timed window holds as many back-to-back calls as fill about this long


def timed(fn, reps):
    """seconds per call: (median, min, max) over `reps` windows, each one event pair around n back-to-back calls"""
    import torch

    def window(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3 / n
    fn()                                               # warm-up: code objects, allocator
    torch.cuda.synchronize()
    n = max(1, min(2000, int(WINDOW_S / max(window(2), 1e-6))))
    out = [window(n) for _ in range(reps)]
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="ml100k,ml1m")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import logging

    import pandas as pd
    import torch
    assert torch.cuda.is_available(), "slim_bench needs a HIP device (there is no CPU path to time)"
    from daisyrec_amd import ops
    from daisyrec_amd.model import SLiM
    dev = "cuda"
    results = {"device": torch.cuda.get_device_name(0)}
    for name in a.sizes.split(","):
        U, I, n = SIZES[name]
        u, i, r = synth(U, I, n)
        alpha, l1r, topk = 1.0, 0.1, 50
        csr = ops.slim_csr(torch.from_numpy(u).to(dev), torch.from_numpy(i).to(dev), torch.from_numpy(r).to(dev), U, I)
        t_gram = timed(lambda: ops.slim_gram(csr, I), a.reps)
        G = ops.slim_gram(csr, I)
        moves = torch.zeros(I, dtype=torch.int64, device=dev)
        t_cd = timed(lambda: ops.slim_fit(G, U, alpha, l1r, topk, moves=moves), a.reps)
        count, rows, vals, sweeps, gap = ops.slim_fit(G, U, alpha, l1r, topk, moves=moves)
        sw, mv = sweeps.cpu().numpy().astype(np.int64), moves.cpu().numpy()
        row_bytes = int(mv.sum()) * I * 4
        sweep_bytes = int(sw.sum()) * 2 * I * 4
        del G
        cfg = dict(gpu="0", alpha=alpha, elastic=l1r, topk=topk, user_num=U, item_num=I, logger=logging.getLogger("slim_bench"))
        frame = pd.DataFrame({"user": u, "item": i, "rating": r})
        SLiM(cfg).fit(frame, verbose=False)            # warm-up: the allocator's first blocks of this size
        fits = []
        for _ in range(5):
            m = SLiM(cfg)
            t0 = time.perf_counter()
            m.fit(frame, verbose=False)                # (ends in the device-to-host copy of fit_info)
            fits.append(time.perf_counter() - t0)
        rng = np.random.RandomState(1)
        loader = [(torch.from_numpy(rng.choice(U, 128, replace=False)), torch.from_numpy(rng.randint(0, I, (128, 1000))))]
        m.rank(loader)
        ranks = []
        for _ in range(max(a.reps, 10)):
            t0 = time.perf_counter()
            m.rank(loader)                             # (returns host ids: synchronised)
            ranks.append(time.perf_counter() - t0)
        t_scores = timed(lambda: ops.slim_scores(m._csr, m._W, I, loader[0][0].to(dev), loader[0][1].to(dev)), a.reps)
        res = dict(users=U, items=I, ratings=int(len(u)), gram_s=t_gram[0], gram_tflops=2.0 * I * I * U / t_gram[0] / 1e12,
                   cd_s=t_cd[0], cd_s_min=t_cd[1], cd_s_max=t_cd[2], sweeps_min=int(sw[sw > 0].min()), sweeps_max=int(sw.max()),
                   sweeps_total=int(sw.sum()), moves_total=int(mv.sum()), nnz_w=int(count.sum()),
                   cd_row_bytes=row_bytes, cd_row_tbs=row_bytes / t_cd[0] / 1e12, cd_sweep_bytes=sweep_bytes,
                   fit_s=statistics.median(fits), rank_128x1000_s=statistics.median(ranks), scores_128x1000_s=t_scores[0])
        results[name] = res
        print(f"== {name}: {U} users x {I} items, {len(u)} ratings; alpha {alpha}, elastic {l1r}, topk {topk}")
        print(f"   gram   {t_gram[0] * 1e3:9.3f} ms (min {t_gram[1] * 1e3:.3f}, max {t_gram[2] * 1e3:.3f})   "
              f"{res['gram_tflops']:.2f} TFLOP/s of 2 I^2 U (dense count; G is {I * I * 4 / 1e6:.1f} MB)")
        print(f"   cd     {t_cd[0] * 1e3:9.3f} ms (min {t_cd[1] * 1e3:.3f}, max {t_cd[2] * 1e3:.3f})   sweeps per column "
              f"{res['sweeps_min']}..{res['sweeps_max']}, {res['moves_total']} coordinate updates, nnz(W) {res['nnz_w']}")
        print(f"          Gram rows read by the H updates: {row_bytes / 1e9:.2f} GB -> {res['cd_row_tbs']:.3f} TB/s "
              f"({100 * res['cd_row_tbs'] / L2_TBS:.1f} % of the L2s' {L2_TBS} TB/s, {100 * res['cd_row_tbs'] / MALL_TBS:.1f} % of the "
              f"Infinity Cache's {MALL_TBS} TB/s, {100 * res['cd_row_tbs'] / HBM_TBS:.1f} % of HBM's {HBM_TBS} TB/s); "
              f"the sweeps' own reads (column j, diagonal): {sweep_bytes / 1e9:.2f} GB more")
        print(f"   fit    {res['fit_s'] * 1e3:9.3f} ms  SLiM.fit(DataFrame), host clock (CSR build, Gram, descent, column form)")
        print(f"   rank   {res['rank_128x1000_s'] * 1e3:9.3f} ms  SLiM.rank, 128 users x 1000 candidates, host clock; the score "
              f"kernel alone {t_scores[0] * 1e6:.1f} us")
    print(json.dumps(results))


if __name__ == "__main__":
    main()
