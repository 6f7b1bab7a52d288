#!/usr/bin/env python
"""Times of DESIGN.md §24 (ops.full_rank_users: fused score, mask and top-k over all items) on the device; writes ONE
JSON object to profiles/bench_full_rank.json (or --out):

    python tools/bench_full_rank.py

Shapes: d = 64, I = 26 744, n in {64, 4096, 138 493} of U = 138 493 users, topk = 50, an exclusion CSR of 20 M distinct
(user, item) entries with Zipf users (exponent 1; a user holds at most the I items there are), and n = U = 6040,
I = 3706 with 1 M entries, where the grid needs several item slices per user tile.  Tables are N(0, 0.1).
Per shape: the time of one call with validate=False (device events around the call, a warm-up call, the median of
--reps timed regions), 2 n I d / t as a fraction of the 155 TF the fp32 MFMA was measured at, the same call without the
exclusion and at topk 1 and 128 (what the mask walk, the appends and the compaction cost), and the route there was
before: a loop of ops.mf_full_rank(u) with its device-to-host copy - the code of `full_rank(u)`, which this change
leaves as it was - timed on --loop-users users with the host clock and EXTRAPOLATED linearly to n (marked as such).
Nothing here is a pass/fail threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from daisyrec_amd import ops  # noqa: E402

DEV = "cuda"
REGION_MS = 50.0
MFMA_F32_PEAK = 155e12         # measured fp32 MFMA rate of the device the kernels are written for


def timed(fn, reps, warm=1):
    """median milliseconds per fn() over `reps` regions between two device events; a region repeats fn() until it
    spans about REGION_MS (a region of one sub-millisecond call would time the clock and the launch queue)"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out, calls = [], 1
    for r in range(reps + 1):               # region 0 sizes the others and is not counted
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / calls
        if r == 0:
            calls = int(min(max(1, np.ceil(REGION_MS / max(ms, 1e-3))), 500))
        else:
            out.append(ms)
    return round(float(np.median(out)), 4)


def zipf_csr(U, I, entries, seed):
    """device CSR of `entries` distinct (user, item) pairs: users log-uniform over [0, U) (Zipf, exponent 1), items uniform"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    draw = int(entries * 1.4)
    while True:
        user = (torch.exp(torch.rand(draw, device=DEV, generator=g, dtype=torch.float64) * np.log(U)).to(torch.int64) - 1).clamp_(0, U - 1)
        item = torch.randint(0, I, (draw,), device=DEV, generator=g)
        key = torch.unique(user * I + item)
        if key.numel() >= entries:
            break
        draw *= 2
    key = key[torch.randperm(key.numel(), device=DEV, generator=g)[:entries]]
    indptr, items = ops.build_user_csr((key // I).to(torch.int32), (key % I).to(torch.int32), U)
    longest = int((indptr[1:] - indptr[:-1]).max().item())
    return (indptr, items), longest


def shape(U, I, d, ns, entries, topk, reps, loop_users, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    P = torch.randn(U, d, device=DEV, generator=g) * 0.1
    Q = torch.randn(I, d, device=DEV, generator=g) * 0.1
    excl, longest = zipf_csr(U, I, entries, seed + 1)
    out = {"users": U, "items": I, "d": d, "topk": topk, "exclusion_entries": int(excl[1].numel()), "longest_exclusion_row": longest,
           "calls": []}
    # the route before: one call, three launches, a radix sort of all I scores and a device-to-host copy per user
    us = torch.randperm(U, device=DEV, generator=g)[:min(loop_users, U)].tolist()
    for u in us[:20]:
        ops.mf_full_rank(P, Q, u, topk).cpu()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for u in us:
        ops.mf_full_rank(P, Q, u, topk).cpu()
    loop_ms_per_user = (time.perf_counter() - t0) * 1e3 / len(us)
    out["loop_full_rank_users_timed"] = len(us)
    out["loop_full_rank_ms_per_user"] = round(loop_ms_per_user, 4)
    for n in ns:
        users = torch.randperm(U, device=DEV, generator=g)[:n].contiguous()
        run = lambda k=topk, ex=excl: ops.full_rank_users(P, Q, users, k, exclude=ex, validate=False)      # noqa: E731
        ms = timed(run, reps)
        ids = run()
        assert ids.shape == (n, topk)
        call = {"n": n, "ms": ms, "lists_with_fewer_eligible_items": int((ids[:, -1] < 0).sum().item()), "mfma_fraction": round(2.0 * n * I * d / (ms * 1e-3) / MFMA_F32_PEAK, 4),
                "workspace_bytes": int(ops.lib.daisy_full_rank_users_workspace_bytes(n, I, topk, 0)),
                "ms_without_exclusion": timed(lambda: run(ex=None), reps),
                "ms_topk_1": timed(lambda: run(k=1), reps), "ms_topk_128": timed(lambda: run(k=128), reps),
                "loop_full_rank_ms_EXTRAPOLATED": round(loop_ms_per_user * n, 2)}
        call["speedup_over_loop"] = round(call["loop_full_rank_ms_EXTRAPOLATED"] / ms, 1)
        out["calls"].append(call)
        print(json.dumps(call), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-users", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_full_rank.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_full_rank needs a HIP device")
    if a.reps < 3 or a.loop_users < 1000:
        raise SystemExit("at least 3 timed regions and 1000 loop users")
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "mfma_f32_peak_flops": MFMA_F32_PEAK,
           "ml20m_shapes": shape(138493, 26744, 64, [64, 4096, 138493], 20_000_000, 50, a.reps, a.loop_users, 0),
           "ml1m_shapes": shape(6040, 3706, 64, [6040], 1_000_000, 50, a.reps, a.loop_users, 10)}
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
