#!/usr/bin/env python
"""Times the stages of EASE on the device (csrc/ease.hip): the Gram matrix, the blocked Cholesky factorisation (potrf), the
blocked inverse (potri: T = L^-1, then P = T^T T), the column scaling and one rank batch (128 users x 1000 candidates), at
ml-100k's shape (943 x 1682, 100 000 ratings), at a synthetic ml-1m-like shape (6040 x 3706, about 1 M ratings) and at one
larger item count (20 000 x 20 000, 2 M ratings), ratings 1..5, ease.yaml's reg = 200.  The data is generated from a seed
(popularity-skewed items); nothing is read from disk.

    python tools/ease_bench.py [--sizes ml100k,ml1m,items20k] [--reps 5] [--out profiles/ease_stages.txt]

Times are device events around windows of back-to-back calls of the stage (about 0.25 s each, at least one call; median,
minimum and maximum of --reps windows after a warm-up call).  potrf works in place, so every timed call first copies the
system back (a device-to-device copy, timed on its own and subtracted).  `fit` is a host clock around EASE.fit(DataFrame),
which ends in a device-to-host copy.  The O(I^3) stages are set against the fp64 matrix rate AMD publishes for the MI355X
(78.6 TFLOP/s; the project's microarchitecture notes carry no fp64 row): potrf counts I^3 / 3 flops, potri 2 I^3 / 3 (the
triangular inverse and the product, I^3 / 3 each).  A factorisation is a chain of about 3 I / 64 dependent launches and
the inverse one of I / 64: at small I the stages are bound by launch latency, not by the matrix pipe.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # the package next to tools/

SIZES = {"ml100k": (943, 1682, 100_000), "ml1m": (6040, 3706, 1_000_000), "items20k": (20_000, 20_000, 2_000_000)}
FP64_MFMA_TFLOPS = 78.6
WINDOW_S = 0.25        # a timed window holds as many back-to-back calls as fill about this long


def synth(U, I, n, seed=0):
    rng = np.random.RandomState(seed)
    pop = rng.zipf(1.3, I).clip(1, 200).astype(float)
    key = np.unique(rng.randint(0, U, 2 * n).astype(np.int64) * I + rng.choice(I, 2 * n, p=pop / pop.sum()))
    key = rng.permutation(key)[:n]
    return key // I, key % I, rng.randint(1, 6, len(key)).astype(np.float64)


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
    n = max(1, min(2000, int(WINDOW_S / max(window(1), 1e-6))))
    out = [window(n) for _ in range(reps)]
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="ml100k,ml1m,items20k")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the text to this file")
    a = ap.parse_args()
    import logging

    import pandas as pd
    import torch
    assert torch.cuda.is_available(), "ease_bench needs a HIP device (there is no CPU path to time)"
    from daisyrec_amd import ops
    from daisyrec_amd.model import EASE
    dev = "cuda"
    results = {"device": torch.cuda.get_device_name(0), "fp64_mfma_peak_tflops": FP64_MFMA_TFLOPS}
    lines = [f"device: {results['device']}; fp64 matrix peak taken as {FP64_MFMA_TFLOPS} TFLOP/s"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for name in a.sizes.split(","):
        U, I, n = SIZES[name]
        free = torch.cuda.mem_get_info()[0]
        if 4 * I * I * 8 + (1 << 30) > free:            # A0, A, T, P at once in this script (a fit holds two)
            say(f"== {name}: skipped, four fp64 [{I} x {I}] buffers do not fit {free / 1e9:.1f} GB free")
            continue
        u, i, r = synth(U, I, n)
        reg = 200.0
        csr = ops.slim_csr(torch.from_numpy(u).to(dev), torch.from_numpy(i).to(dev), torch.from_numpy(r).to(dev), U, I)
        t_gram = timed(lambda: ops.slim_gram(csr, I), a.reps)
        A0 = ops.ease_system(ops.slim_gram(csr, I), reg)
        A = torch.empty_like(A0)
        ws = ops.ease_workspace(I, dev)
        t_copy = timed(lambda: A.copy_(A0), a.reps)
        t_potrf_c = timed(lambda: ops.ease_potrf(A.copy_(A0), ws), a.reps)
        _, info, _ = ops.ease_potrf(A.copy_(A0), ws)
        assert int(info.item()) == 0
        t_potrf = tuple(max(x - t_copy[0], 0.0) for x in t_potrf_c)
        t_potri = timed(lambda: ops.ease_potri(A, ws), a.reps)
        P = ops.ease_potri(A, ws)
        del A0
        t_w = timed(lambda: ops.ease_weights(P, ws), a.reps)
        Bm = ops.ease_weights(P, ws, inplace=True)
        del A
        rng = np.random.RandomState(1)
        us = torch.from_numpy(rng.choice(U, 128, replace=False)).to(dev)
        cands = torch.from_numpy(rng.randint(0, I, (128, 1000))).to(dev)
        t_rank = timed(lambda: ops.ease_rank(csr, Bm, us, cands, 50), a.reps)
        t_full = timed(lambda: ops.ease_rank(csr, Bm, us, None, 50), a.reps)
        del Bm, P
        cfg = dict(gpu="0", reg=reg, topk=50, user_num=U, item_num=I, UID_NAME="user", IID_NAME="item", INTER_NAME="rating",
                   logger=logging.getLogger("ease_bench"))
        frame = pd.DataFrame({"user": u, "item": i, "rating": r})
        EASE(cfg).fit(frame)                            # warm-up: the allocator's first blocks of this size
        fits = []
        for _ in range(3):
            m = EASE(cfg)
            t0 = time.perf_counter()
            m.fit(frame)                                # (ends in the device-to-host copy of info)
            fits.append(time.perf_counter() - t0)
        del m
        torch.cuda.empty_cache()
        f3 = I ** 3 / 3.0
        res = dict(users=U, items=I, ratings=int(len(u)), gram_s=t_gram[0], copy_s=t_copy[0], potrf_s=t_potrf[0],
                   potrf_tflops=f3 / max(t_potrf[0], 1e-12) / 1e12, potri_s=t_potri[0], potri_tflops=2 * f3 / t_potri[0] / 1e12,
                   weights_s=t_w[0], rank_128x1000_s=t_rank[0], full_rank_128_s=t_full[0], fit_s=statistics.median(fits),
                   launches_potrf=3 * ((I + 63) // 64) - 2, launches_potri=(I + 63) // 64 + 1)
        results[name] = res
        say(f"== {name}: {U} users x {I} items, {len(u)} ratings; reg {reg}; one fp64 [I, I] buffer is {I * I * 8 / 1e6:.1f} MB")
        say(f"   gram    {t_gram[0] * 1e3:10.3f} ms (min {t_gram[1] * 1e3:.3f}, max {t_gram[2] * 1e3:.3f})")
        say(f"   potrf   {t_potrf[0] * 1e3:10.3f} ms (min {t_potrf[1] * 1e3:.3f}, max {t_potrf[2] * 1e3:.3f}; the copy of "
            f"{t_copy[0] * 1e3:.3f} ms subtracted)   {res['launches_potrf']} launches, {t_potrf[0] / res['launches_potrf'] * 1e6:.1f} us "
            f"each; I^3/3 = {f3 / 1e9:.2f} GFLOP -> {res['potrf_tflops']:.3f} TFLOP/s = "
            f"{100 * res['potrf_tflops'] / FP64_MFMA_TFLOPS:.2f} % of {FP64_MFMA_TFLOPS}")
        say(f"   potri   {t_potri[0] * 1e3:10.3f} ms (min {t_potri[1] * 1e3:.3f}, max {t_potri[2] * 1e3:.3f})   "
            f"{res['launches_potri']} launches; 2 I^3/3 = {2 * f3 / 1e9:.2f} GFLOP -> {res['potri_tflops']:.3f} TFLOP/s = "
            f"{100 * res['potri_tflops'] / FP64_MFMA_TFLOPS:.2f} % of {FP64_MFMA_TFLOPS}")
        say(f"   weights {t_w[0] * 1e3:10.3f} ms (min {t_w[1] * 1e3:.3f}, max {t_w[2] * 1e3:.3f})   "
            f"{2 * I * I * 8 / t_w[0] / 1e12:.2f} TB/s read + written")
        say(f"   rank    {t_rank[0] * 1e3:10.3f} ms  128 users x 1000 candidates, top 50; over all {I} items {t_full[0] * 1e3:.3f} ms")
        say(f"   fit     {res['fit_s'] * 1e3:10.3f} ms  EASE.fit(DataFrame), host clock (CSR build, Gram, system, potrf, potri, weights)")
    print(json.dumps(results))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
