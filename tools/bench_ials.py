#!/usr/bin/env python
"""Times of DESIGN.md §29 (iALS: Gram matrix, half-sweeps, objective) on the device; prints ONE JSON line (kept under
profiles/):

    python tools/bench_ials.py > profiles/bench_ials.json

Synthetic interactions, users and items uniform (so row lengths are near their mean: skewed row lengths are NOT measured
here), ratings 1..5, tables normal(0, 0.1), alpha = 10, reg = 0.1, at
  * ml-20m shapes (138 493 x 26 744, 20 M interactions), d = 64 and d = 128;
  * BASELINE configs[1] shapes (1 M x 100 K, 50 M interactions), d = 64.
Per half-sweep (Gram matrix included, as a fit runs it): the time between two device events, the median of `reps`
repetitions after a warm-up call; nnz * d * 4 gathered bytes over that time, beside the library's own measured rate for
random 256-byte rows (README: 4.8 TB/s); the fp64 flops the kernel executes over that time - 2 * 16 * 16 * 4 per MFMA
instruction, one per tile of the lower triangle and four entries (rows padded to a multiple of four), plus d^3 / 3 + 2 d^2
per factored row.  The objective kernel likewise.  A CPU leg: the same half-sweep in numpy fp64 on a few thousand rows of
the same data, EXTRAPOLATED per row (marked as such).  Nothing here is a pass/fail threshold.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from daisyrec_amd import ops  # noqa: E402

DEV = "cuda"
ALPHA, REG = 10.0, 0.1
RANDOM_ROW_TB_S = 4.8          # README: gather of random 256-byte rows, measured by tools/membench.py
SHAPES = [("ml-20m", 138_493, 26_744, 20_000_000, 64), ("BASELINE configs[1]", 1_000_000, 100_000, 50_000_000, 64),
          ("ml-20m", 138_493, 26_744, 20_000_000, 128)]


def timed(fn, reps, warm=1):
    """median milliseconds between two device events around fn()"""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return round(float(np.median(out)), 3)


def flops(row_ptr, d):
    lens = (row_ptr[1:] - row_ptr[:-1])
    t = (d + 15) // 16
    mfma = int(((lens + 3) // 4).sum().item()) * (t * (t + 1) // 2) * 2 * 16 * 16 * 4
    solve = int((lens > 0).sum().item()) * (d ** 3 // 3 + 2 * d * d)
    return mfma, solve


def side(csr, other, reps):
    d = other.shape[1]
    nnz = int(csr[1].numel())
    out = torch.empty(csr[0].numel() - 1, d, dtype=torch.float32, device=DEV)
    ms = timed(lambda: ops.ials_half_sweep(csr, other, ALPHA, REG, out=out, validate=False), reps)
    gram_ms = timed(lambda: ops.ials_gram(other), reps)
    mfma, solve = flops(csr[0], d)
    gathered = nnz * d * 4
    return out, {"rows": int(csr[0].numel() - 1), "ms": ms, "gram_ms_of_it": gram_ms,
                 "gathered_gb": round(gathered / 1e9, 2), "gathered_tb_per_s": round(gathered / (ms * 1e-3) / 1e12, 3),
                 "random_row_rate_tb_per_s_for_comparison": RANDOM_ROW_TB_S,
                 "fp64_gflop_mfma": round(mfma / 1e9, 1), "fp64_gflop_cholesky_and_solves": round(solve / 1e9, 1),
                 "fp64_tflop_per_s": round((mfma + solve) / (ms * 1e-3) / 1e12, 2)}


def cpu_leg(csr, other, rows):
    """numpy fp64 on the first `rows` rows: seconds, and the whole half-sweep EXTRAPOLATED per row"""
    row_ptr, col, val = (t.cpu().numpy() for t in csr)
    Y = other.cpu().numpy().astype(np.float64)
    d = Y.shape[1]
    t0 = time.perf_counter()
    G = Y.T @ Y + REG * np.eye(d)
    for u in range(rows):
        Yu = Y[col[row_ptr[u]:row_ptr[u + 1]]]
        w = ALPHA * val[row_ptr[u]:row_ptr[u + 1]].astype(np.float64)
        np.linalg.solve(G + (Yu * w[:, None]).T @ Yu, ((1.0 + w)[:, None] * Yu).sum(0))
    s = time.perf_counter() - t0
    total = len(row_ptr) - 1
    return {"rows_timed": rows, "seconds_timed": round(s, 3), "threads": torch.get_num_threads(),
            "half_sweep_seconds_EXTRAPOLATED": round(s / rows * total, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-rows", type=int, default=4000)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink every shape (a quick look, not the recorded run)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ials needs a HIP device")
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "alpha": ALPHA, "reg": REG, "row_lengths": "uniform",
           "shapes": []}
    for name, U, I, n, d in SHAPES:
        U, I, n = (max(int(x * a.scale), 16) for x in (U, I, n))
        g = torch.Generator(device=DEV).manual_seed(0)
        u = torch.randint(0, U, (n,), device=DEV, generator=g)
        i = torch.randint(0, I, (n,), device=DEV, generator=g)
        r = torch.randint(1, 6, (n,), device=DEV, generator=g).to(torch.float64)
        csr, csr_t = ops.slim_csr(u, i, r, U, I), ops.slim_csr(i, u, r, I, U)
        del u, i, r
        P = 0.1 * torch.randn(U, d, device=DEV, generator=g)
        Q = 0.1 * torch.randn(I, d, device=DEV, generator=g)
        rec = {"shape": name, "users": U, "items": I, "d": d, "nnz": int(csr[1].numel()),
               "longest_user_row": int((csr[0][1:] - csr[0][:-1]).max().item()),
               "longest_item_row": int((csr_t[0][1:] - csr_t[0][:-1]).max().item())}
        P, rec["user_half_sweep"] = side(csr, Q, a.reps)
        Q, rec["item_half_sweep"] = side(csr_t, P, a.reps)
        G = ops.ials_gram(Q)
        rec["objective_ms"] = timed(lambda: ops.ials_objective(csr, P, Q, ALPHA, REG, G=G), a.reps)
        rec["objective"] = float(ops.ials_objective(csr, P, Q, ALPHA, REG, G=G).item())
        rec["cpu_numpy_user_half_sweep"] = cpu_leg(csr, Q, min(a.cpu_rows, U))
        out["shapes"].append(rec)
        print(f"{name} d={d} done", file=sys.stderr, flush=True)
        del csr, csr_t, P, Q
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
