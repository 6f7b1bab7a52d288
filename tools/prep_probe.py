#!/usr/bin/env python
"""Times of DESIGN.md §21 (Preprocessor and splitters) on the device; prints plain lines (kept under profiles/):

    python tools/prep_probe.py > profiles/prep_probe.txt

Synthetic interactions: 50 M rows, 1 M users (uniform), 100 K items (Zipf with exponent 1: log-uniform ranks), distinct
timestamps in random order, so about 50 rows per user and a few per cent duplicated pairs.  Timed, on device-resident
columns (the host's DataFrame gather and the copies to and from the device are not part of these numbers):
  * `daisy_prep_process`, 5core / ui with item_pop, and the peel rounds it took;
  * `daisy_prep_encode` of the user column (what every per-user split starts with);
  * `daisy_split_ids` for tloo, utfo, ufo, rloo and rsbr.
Every entry ends in a stream synchronise, so the host clock around a call is the call.  Each line: the median of 15
timed regions after 2 warm-up calls, with the minimum and the maximum.  Nothing here is a pass/fail threshold.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from daisyrec_amd import ops  # noqa: E402

DEV = "cuda"


def timed(fn, reps=15, warm=2):
    """median / min / max milliseconds of fn(), host clock around a call that synchronises"""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prep_probe needs a HIP device")
    n, U, I = a.rows, a.users, a.items
    print(torch.cuda.get_device_name(0), f"rows={n} users={U} items={I} (Zipf)")
    g = torch.Generator(device=DEV).manual_seed(0)
    users = torch.randint(0, U, (n,), device=DEV, generator=g) * 7 + 11
    items = (torch.exp(torch.rand(n, device=DEV, generator=g, dtype=torch.float64) * np.log(I)).to(torch.int64) - 1).clamp_(0, I - 1)
    ts = torch.randperm(n, device=DEV, generator=g)
    rating = torch.ones(n, device=DEV, dtype=torch.float64)

    def line(what, fn, rows=n):
        med, lo, hi = timed(fn)
        print(f"{what}: {med:.1f} ms median of 15 (min {lo:.1f}, max {hi:.1f}); {med * 1e6 / rows:.2f} ns per row")

    out = ops.prep_process(users, items, rating, ts, mode="core", level="ui", N=5, want_pop=True)
    print(f"5core / ui: {n} rows -> {out['rows'].numel()}, {out['user_num']} users, {out['item_num']} items, "
          f"{out['rounds']} peel rounds")
    line("prep_process 5core / ui + item_pop", lambda: ops.prep_process(users, items, rating, ts, mode="core", level="ui", N=5,
                                                                        want_pop=True))
    line("prep_process origin (encode, dedup, recode, time sort)", lambda: ops.prep_process(users, items, None, ts))
    df_user = users[out["rows"]].contiguous()                # the split works on the processed frame, in time order
    df_ts = ts[out["rows"]].contiguous()
    m = df_user.numel()
    code, tok = ops.prep_encode(df_user)
    line(f"prep_encode, {m} rows", lambda: ops.prep_encode(df_user), m)
    for method in ("tloo", "utfo", "ufo", "rloo", "rsbr"):
        tr, te = ops.split_ids(method, m, code, tok.numel(), df_ts, size=0.2, seed=2022)
        line(f"split_ids {method}, {m} rows -> {te.numel()} test", lambda: ops.split_ids(method, m, code, tok.numel(), df_ts,
                                                                                     size=0.2, seed=2022), m)


if __name__ == "__main__":
    main()
