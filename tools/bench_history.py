#!/usr/bin/env python
"""Times of DESIGN.md §23 (history matrix, its direct CSR, first-seen order) on the device; prints ONE JSON line (kept
under profiles/):

    python tools/bench_history.py > profiles/bench_history.json

Synthetic interactions: `--rows` rows (default 50 M), one user per 50 rows with Zipf popularity (exponent 1: log-uniform
ranks, so the heaviest user holds about rows / ln(users) of them), 100 K items, values 1..5.  Timed on device-resident
code columns (the host's DataFrame access and the copy to the device are not part of these numbers):
  * `history_csr` and `history_first_seen` at the full size - they are bounded by the interactions;
  * `history_counts` + `history_fill` (the padded pair) at the largest power of ten of rows, from --rows down, at which
    users x longest x 12 bytes fits the device's free memory, and `history_csr` at that size too;
  * the route to the same CSR before csrc/history.hip: the two host loops of get_history_matrix, written out below, timed
    on at most 1 M rows and EXTRAPOLATED per row to the size in question (marked as such), followed by
    `ops.vae_history_csr` on the padded pair, at the largest size where its temporaries fit.
Every entry ends in a stream synchronise, so the host clock around a call is the call.  Each time: the median of `reps`
timed regions after a warm-up call.  Nothing here is a pass/fail threshold.
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
HOST_LOOP_ROWS = 1_000_000


def timed(fn, reps=5, warm=1):
    """median milliseconds of fn(), host clock around a call that synchronises"""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(out)), 3)


def frame(n, items, seed=0):
    """(user int32 [n], item int32 [n], value float64 [n], user_num) on the device"""
    U = max(n // 50, 2)
    g = torch.Generator(device=DEV).manual_seed(seed)
    user = (torch.exp(torch.rand(n, device=DEV, generator=g, dtype=torch.float64) * np.log(U)).to(torch.int64) - 1).clamp_(0, U - 1)
    item = torch.randint(0, items, (n,), device=DEV, generator=g)
    val = torch.randint(1, 6, (n,), device=DEV, generator=g).to(torch.float64)
    return user.to(torch.int32), item.to(torch.int32), val, U


def host_loops(row_ids, col_ids, values, row_num):
    """the two loops over the rows of the frame: a count per row, then every entry into its row's next free place"""
    lens = np.zeros(row_num, dtype=np.int64)
    for r in row_ids:
        lens[r] += 1
    width = int(lens.max())
    ids = np.zeros((row_num, width), dtype=np.int64)
    vals = np.zeros((row_num, width))
    lens[:] = 0
    for r, v, c in zip(row_ids, values, col_ids):
        ids[r, lens[r]] = c
        vals[r, lens[r]] = v
        lens[r] += 1
    return ids, vals, lens


def free_bytes():
    return torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved() - torch.cuda.memory_allocated()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_history needs a HIP device")
    out = {"device": torch.cuda.get_device_name(0), "items": a.items, "reps": a.reps, "users_per_row": 1 / 50}

    # ---- bounded by the interactions: the full size
    n = a.rows
    user, item, val, U = frame(n, a.items)
    row_ptr, col, _, L = ops.history_csr(user, item, val, U, a.items)
    full = {"rows": n, "users": U, "longest": L, "nnz": int(col.numel()), "padded_bytes": U * L * 12,
            "csr_bytes": int((U + 1) * 8 + col.numel() * 8),
            "history_csr_ms": timed(lambda: ops.history_csr(user, item, val, U, a.items, validate=False), a.reps),
            "first_seen_users_ms": timed(lambda: ops.history_first_seen(user, U, validate=False), a.reps),
            "first_seen_items_ms": timed(lambda: ops.history_first_seen(item, a.items, validate=False), a.reps),
            "history_counts_ms": timed(lambda: ops.history_counts(user, U, validate=False), a.reps)}
    out["full"] = full
    print("full size done", file=sys.stderr, flush=True)
    del user, item, val, row_ptr, col
    torch.cuda.empty_cache()

    # ---- the padded pair: the largest power of ten of rows at which it fits
    sizes = [n] + [10 ** e for e in range(int(np.ceil(np.log10(n))) - 1, 2, -1)]
    tried = []
    for m in sizes:
        user, item, val, U = frame(m, a.items)
        hlen, L, order, start = ops.history_counts(user, U, validate=False)
        need = U * L * 12
        tried.append({"rows": m, "users": U, "longest": L, "padded_bytes": need})
        if need * 1.05 + (1 << 30) < free_bytes():
            break
        del user, item, val, hlen, order, start
        torch.cuda.empty_cache()
    else:
        raise SystemExit("no size fits: " + json.dumps(tried))
    pad = dict(tried[-1])
    pad["history_counts_ms"] = timed(lambda: ops.history_counts(user, U, validate=False), a.reps)
    pad["history_fill_ms"] = timed(lambda: ops.history_fill(order, start, item, val, U, L), a.reps)
    pad["fill_store_gb_per_s"] = round(need / (pad["history_fill_ms"] * 1e-3) / 1e9, 1)
    pad["history_csr_ms"] = timed(lambda: ops.history_csr(user, item, val, U, a.items, validate=False), a.reps)
    pad["sizes_that_did_not_fit"] = tried[:-1]
    out["padded"] = pad
    print("padded pair done", file=sys.stderr, flush=True)

    # ---- the route before: host loops (timed on <= 1 M rows, extrapolated per row) + ops.vae_history_csr of the pair
    # (the loops' cost per row does not depend on who owns the row: they are timed on uniform users, whose padded pair
    # is small enough for the host)
    k = min(n, HOST_LOOP_ROWS)
    rng = np.random.default_rng(0)
    hu, hi, hv = rng.integers(0, k // 50, k), rng.integers(0, a.items, k), rng.integers(1, 6, k).astype(np.float64)
    t0 = time.perf_counter()
    host_loops(hu, hi, hv, k // 50)
    loops_s = time.perf_counter() - t0
    before = {"host_loops_rows_timed": k, "host_loops_frame": "uniform users", "host_loops_s_timed": round(loops_s, 3),
              "host_loops_ns_per_row": round(loops_s / k * 1e9, 1),
              "host_loops_s_at_padded_rows_EXTRAPOLATED": round(loops_s / k * m, 3),
              "host_loops_s_at_full_rows_EXTRAPOLATED": round(loops_s / k * n, 1)}
    del hlen, order, start
    vm, vuser, vitem, vval, vU = m, user, item, val, U
    while vm >= 1000:
        try:
            _, vL, vorder, vstart = ops.history_counts(vuser, vU, validate=False)
            hid, hvl = ops.history_fill(vorder, vstart, vitem, vval, vU, vL)
            del vorder, vstart
            before["vae_history_csr_ms"] = timed(lambda: ops.vae_history_csr(hid, hvl, a.items), max(a.reps // 2, 1))
            before.update({"vae_history_csr_rows": vm, "vae_history_csr_cells": vU * vL})
            before["history_csr_ms_same_rows"] = timed(lambda: ops.history_csr(vuser, vitem, vval, vU, a.items, validate=False),
                                                       a.reps)
            break
        except torch.cuda.OutOfMemoryError:
            before.setdefault("vae_history_csr_out_of_memory_at_rows", []).append(vm)
            hid = hvl = None
            torch.cuda.empty_cache()
            vm //= 10
            vuser, vitem, vval, vU = frame(vm, a.items)
    out["before"] = before
    print(json.dumps(out))


if __name__ == "__main__":
    main()
