#!/usr/bin/env python
"""Times of DESIGN.md §30 (the two-hop walk with a per-row top-K, and RP3beta's whole fit) on the device; prints ONE JSON
line (kept under profiles/):

    python tools/bench_rp3.py > profiles/bench_rp3.json

Synthetic interactions at ml-20m shapes (138 493 x 26 744, 20 M draws) and ml-1m shapes (6 040 x 3 706, 1 M draws), users
and items drawn uniformly or both from a Zipf law (exponent 1: a few very long rows, as real data has); duplicate pairs
collapse, so nnz is below the draws.  Per case, between two device events, the median of `reps` repetitions after a
warm-up call (fewer repetitions when the warm-up call alone took seconds: the count used is recorded):
  * walk: ops.walk2_topk on RP3beta's operands, K = 100 - with paths = sum_u deg(u)^2, paths / s and the peak of the
    device allocator above what was held before the call;
  * heaviest_row: the same walk on the ONE longest source row (a row is one workgroup's, so this is serial time);
  * fit: RP3beta.fit on the DataFrame (host checks, upload, both CSRs, the powers, the walk, the transposes);
  * knn_fit: ops.knn_fit(..., 'cosine') on the same CSR in the same process - the dense-Gram route every other item-item
    model here takes - with its peak likewise.
Nothing here is a pass/fail threshold.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from daisyrec_amd import ops  # noqa: E402
from daisyrec_amd.model import RP3beta  # noqa: E402

DEV = "cuda"
K, ALPHA, BETA = 100, 1.0, 0.6
SHAPES = [("ml-1m", 6_040, 3_706, 1_000_000), ("ml-20m", 138_493, 26_744, 20_000_000)]


def timed(fn, reps):
    """(median milliseconds between two device events around fn(), the repetitions used)"""
    def once():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)
    warm = once()
    reps = reps if warm < 1500 else (3 if warm < 6000 else 1)
    return round(float(np.median([once() for _ in range(reps)])), 3), reps


def peak_of(fn):
    """bytes the device allocator peaked at during fn() above what was allocated before it"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - before)


def draw(n_ids, n, zipf, g):
    if not zipf:
        return torch.randint(0, n_ids, (n,), device=DEV, generator=g)
    cdf = torch.cumsum(1.0 / torch.arange(1, n_ids + 1, device=DEV, dtype=torch.float64), 0)
    ids = torch.searchsorted(cdf / cdf[-1], torch.rand(n, device=DEV, dtype=torch.float64, generator=g))
    return ids.clamp_(max=n_ids - 1)


def one_row(csr, row):
    lo, hi = int(csr[0][row].item()), int(csr[0][row + 1].item())
    ptr = torch.tensor([0, hi - lo], dtype=torch.int64, device=DEV)
    return ptr, csr[1][lo:hi].contiguous(), csr[2][lo:hi].contiguous()


def case(name, U, I, n, zipf, reps):
    import pandas as pd
    g = torch.Generator(device=DEV).manual_seed(0)
    u, i = draw(U, n, zipf, g), draw(I, n, zipf, g)
    pair = torch.unique(u * I + i)                              # duplicate pairs collapse: implicit feedback
    u, i = pair // I, pair % I
    frame = pd.DataFrame({"user": u.cpu().numpy(), "item": i.cpu().numpy(), "rating": np.ones(u.numel())})
    model = RP3beta({"gpu": "0", "user_num": U, "item_num": I, "topk": 10, "maxk": K, "alpha": ALPHA, "beta": BETA})
    fit_ms, fit_reps = timed(lambda: model.fit(frame), reps)
    Piu, Pui = model._P
    col_scale = model.scales[2]
    csr = model._csr
    k = min(K, I)
    deg_u, deg_i = csr[0][1:] - csr[0][:-1], Piu[0][1:] - Piu[0][:-1]
    paths = int((deg_u * deg_u).sum().item())
    rec = {"shape": name, "row_lengths": "zipf" if zipf else "uniform", "users": U, "items": I, "nnz": int(csr[1].numel()),
           "K": k, "longest_user_row": int(deg_u.max().item()), "longest_item_row": int(deg_i.max().item()), "paths": paths}

    def walk():
        return ops.walk2_topk(Piu, Pui, I, k, col_scale, validate=False)

    ms, r = timed(walk, reps)
    rec["walk"] = {"ms": ms, "reps": r, "paths_per_s": round(paths / (ms * 1e-3), 0), "peak_bytes": peak_of(walk),
                   "path": "lds" if I <= ops.N.WALK2_LDS_COLS else "global"}
    heavy = int(torch.argmax(deg_i).item())
    row = one_row(Piu, heavy)
    row_paths = int(deg_u[row[1].to(torch.int64)].sum().item())
    ms, r = timed(lambda: ops.walk2_topk(row, Pui, I, k, col_scale, zero_diagonal=False, validate=False), reps)
    rec["heaviest_row"] = {"item": heavy, "entries": int(row[1].numel()), "paths": row_paths, "ms": ms, "reps": r,
                           "paths_per_s": round(row_paths / (ms * 1e-3), 0)}
    rec["fit"] = {"ms": fit_ms, "reps": fit_reps, "bytes_held": model.fit_info["bytes_held"]}

    def knn():
        return ops.knn_fit(csr, I, "cosine", 0.0, k, normalize=True)

    ms, r = timed(knn, reps)
    rec["knn_fit_cosine"] = {"ms": ms, "reps": r, "peak_bytes": peak_of(knn),
                             "dense_flops": 2 * U * I * I, "daisy_knn_fit_bytes": int(ops.lib.daisy_knn_fit_bytes(U, I, k))}
    rec["walk_over_knn_fit"] = round(rec["walk"]["ms"] / ms, 4)
    rec["verdict"] = "walk wins" if rec["walk"]["ms"] < ms else "walk LOSES"
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink every shape (a quick look, not the recorded run)")
    ap.add_argument("--only", default="", help="comma list of shape:dist to run, e.g. ml-1m:zipf")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rp3 needs a HIP device")
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "alpha": ALPHA, "beta": BETA, "cases": []}
    for name, U, I, n in SHAPES:
        U, I, n = (max(int(x * a.scale), 16) for x in (U, I, n))
        for zipf in (False, True):
            tag = f"{name}:{'zipf' if zipf else 'uniform'}"
            if a.only and tag not in a.only.split(","):
                continue
            out["cases"].append(case(name, U, I, n, zipf, a.reps))
            print(f"{tag} done: {json.dumps(out['cases'][-1])}", file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
