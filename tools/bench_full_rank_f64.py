#!/usr/bin/env python
"""Times of DESIGN.md §25 (ops.{ease,slim,knn,psvd}_full_rank_users: the model's fp64 score, the exclusion mask and a
streaming top-k in one launch) on the device; writes ONE JSON object to profiles/bench_full_rank_f64.json (or --out):

    python tools/bench_full_rank_f64.py

Shapes: ml-1m (6040 x 3706, 1 M entries) for EASE, SLiM, ItemKNN, UserKNN and PureSVD; ml-20m (138 493 x 26 744, 20 M
entries) for PureSVD, ItemKNN (40 per column) and a SLiM-like sparse W (50 per column); EASE at ml-20m on a SLICE of
4096 users (W alone is 5.7 GB).  Operands are synthetic - Zipf users, ratings 1..5, N(0, 1) weights: fitting is not what
is timed.  topk = 50, the exclusion is X's own CSR (the training items).
Per shape and n: the time of one *_full_rank_users call with validate=False, the output allocation included (device
events around the call, a warm-up call, the median of --reps timed regions), and the two routes there were before, both
the code this change leaves as it was: a loop of one-user ops.*_rank(..., None, topk) calls with the device-to-host copy
- `full_rank(u)`, which excludes nothing - timed on --loop-users users with the host clock and EXTRAPOLATED linearly to
n (marked as such), and the batched ops.*_rank(users, None, topk), which writes the [n, I] score matrix first, timed
where that matrix fits in 8 GB.  Nothing here is a pass/fail threshold."""
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
MATRIX_BYTES_MAX = 8 << 30
TOPK = 50


def timed(fn, reps, warm=1):
    """median milliseconds per fn() over `reps` regions between two device events; a region repeats fn() until it
    spans about REGION_MS (tools/bench_full_rank.py's)"""
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


def zipf_pairs(U, I, entries, g):
    """`entries` distinct (user, item) pairs: users log-uniform over [0, U) (Zipf, exponent 1), items uniform"""
    draw = int(entries * 1.4)
    while True:
        user = (torch.exp(torch.rand(draw, device=DEV, generator=g, dtype=torch.float64) * np.log(U)).to(torch.int64) - 1).clamp_(0, U - 1)
        item = torch.randint(0, I, (draw,), device=DEV, generator=g)
        key = torch.unique(user * I + item)
        if key.numel() >= entries:
            break
        draw *= 2
    key = key[torch.randperm(key.numel(), device=DEV, generator=g)[:entries]]
    return key // I, key % I


def sparse_by_column(inner, n_cols, per_col, g):
    """(ptr, row, val): per_col distinct ascending rows in every column (an arithmetic progression modulo inner)"""
    per_col = min(per_col, inner)
    start = torch.randint(0, inner, (n_cols, 1), device=DEV, generator=g)
    step = torch.randint(1, max(2, inner // per_col + 1), (n_cols, 1), device=DEV, generator=g)
    rows = (start + step * torch.arange(per_col, device=DEV)) % inner
    rows = torch.sort(rows, dim=1).values.to(torch.int32).reshape(-1).contiguous()
    ptr = torch.arange(n_cols + 1, device=DEV, dtype=torch.int64) * per_col
    return ptr, rows, torch.randn(n_cols * per_col, device=DEV, generator=g)


def model_calls(name, U, I, X, Xt, g, factors):
    """(new(users, exclude), old(users, topk) -> (scores, ids), bytes one user reads from the weights) of a model"""
    if name == "ease":
        W = torch.randn(I, I, device=DEV, generator=g, dtype=torch.float64)
        hist = float((X[0][1:] - X[0][:-1]).double().mean().item())
        return (lambda us, ex: ops.ease_full_rank_users(X, W, us, TOPK, exclude=ex, validate=False),
                lambda us, k: ops.ease_rank(X, W, us, None, k), hist * I * 8)
    if name == "psvd":
        uv = torch.randn(U, factors, device=DEV, generator=g, dtype=torch.float64)
        iv = torch.randn(I, factors, device=DEV, generator=g, dtype=torch.float64)
        return (lambda us, ex: ops.psvd_full_rank_users(uv, iv, us, TOPK, exclude=ex, validate=False),
                lambda us, k: ops.psvd_rank(uv, iv, us, None, k), I * factors * 8)
    if name == "slim":
        W = sparse_by_column(I, I, 50, g)
        return (lambda us, ex: ops.slim_full_rank_users(X, W, I, us, TOPK, exclude=ex, validate=False),
                lambda us, k: (ops.slim_scores(X, W, I, us), None), I * 50 * 8)
    if name == "itemknn":
        W = sparse_by_column(I, I, 40, g)
        return (lambda us, ex: ops.knn_full_rank_users(X, W, I, I, us, TOPK, exclude=ex, validate=False),
                lambda us, k: ops.knn_rank(X, W, I, I, us, None, k), I * 40 * 8)
    S = sparse_by_column(U, U, 40, g)          # userknn: the similarity's rows (a CSR over users), X by column
    per_col = float((Xt[0][1:] - Xt[0][:-1]).double().mean().item())
    return (lambda us, ex: ops.knn_full_rank_users(S, Xt, U, I, us, TOPK, exclude=ex, validate=False),
            lambda us, k: ops.knn_rank(S, Xt, U, I, us, None, k), I * per_col * 8)


def shape(tag, U, I, entries, models, ns, reps, loop_users, seed, factors=150):
    g = torch.Generator(device=DEV).manual_seed(seed)
    users, items = zipf_pairs(U, I, entries, g)
    ratings = torch.randint(1, 6, (entries,), device=DEV, generator=g).double()
    X = ops.slim_csr(users, items, ratings, U, I)
    Xt = ops.slim_csr(items, users, ratings, I, U) if "userknn" in models else None
    excl = (X[0], X[1])
    out = {"users": U, "items": I, "entries": entries, "topk": TOPK, "models": {}}
    for name, n_list in models.items():
        new, old, weight_bytes = model_calls(name, U, I, X, Xt, g, factors)
        rec = {"weight_bytes_read_per_user": int(weight_bytes), "calls": []}
        if name == "slim":                      # slim_scores selects nothing: the loop adds full_topk_from_scores, as full_rank does
            one = lambda u: ops.full_topk_from_scores(old(u, TOPK)[0].view(-1), TOPK).cpu()       # noqa: E731
        else:
            one = lambda u: old(u, TOPK)[1].cpu()                                                  # noqa: E731
        us = torch.randperm(U, device=DEV, generator=g)[:min(loop_users, U)]
        singles = [us[j:j + 1].contiguous() for j in range(us.numel())]
        for u in singles[:20]:
            one(u)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for u in singles:
            one(u)
        loop_ms = (time.perf_counter() - t0) * 1e3 / len(singles)
        rec["loop_full_rank_users_timed"] = len(singles)
        rec["loop_full_rank_ms_per_user"] = round(loop_ms, 4)
        for n in (n_list or ns):
            sel = torch.randperm(U, device=DEV, generator=g)[:n].contiguous()
            ms = timed(lambda: new(sel, excl), reps)
            ids = new(sel, excl)
            assert ids.shape == (n, TOPK)
            call = {"n": n, "ms": ms, "ms_without_exclusion": timed(lambda: new(sel, None), reps),
                    "lists_with_fewer_eligible_items": int((ids[:, -1] < 0).sum().item()),
                    "weight_GB_per_s": round(weight_bytes * n / (ms * 1e-3) / 1e9, 1),
                    "loop_full_rank_ms_EXTRAPOLATED": round(loop_ms * n, 2)}
            if n * I * 8 <= MATRIX_BYTES_MAX:
                call["batched_rank_ms"] = timed(lambda: old(sel, TOPK), max(3, reps - 2))
                call["batched_rank_matrix_bytes"] = n * I * (4 if name == "slim" else 8)
                if name == "slim":
                    call["batched_rank_note"] = "slim_scores only: the existing path has no batched top-k"
            best = min(call["loop_full_rank_ms_EXTRAPOLATED"], call.get("batched_rank_ms", float("inf")))
            call["ratio_to_faster_baseline"] = round(best / ms, 2)
            rec["calls"].append(call)
            print(tag, name, json.dumps(call), file=sys.stderr, flush=True)
        out["models"][name] = rec
        del new, old, one
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-users", type=int, default=1000)
    ap.add_argument("--only", choices=["ml1m", "ml20m", "ease20m"], default=None)
    ap.add_argument("--models", default=None, help="comma-separated subset of the models (a narrow run under a kernel trace)")
    ap.add_argument("--ns", default=None, help="comma-separated user counts instead of the shape's own")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_full_rank_f64.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_full_rank_f64 needs a HIP device")
    if a.reps < 3 or a.loop_users < 1000:
        raise SystemExit("at least 3 timed regions and 1000 loop users")
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "matrix_bytes_max": MATRIX_BYTES_MAX}
    fit20 = MATRIX_BYTES_MAX // (26744 * 8)            # the largest n whose [n, I] fp64 matrix fits
    ns = [int(x) for x in a.ns.split(",")] if a.ns else None
    pick = lambda names: dict.fromkeys(m for m in names if a.models is None or m in a.models.split(","))      # noqa: E731
    if a.only in (None, "ml1m"):
        out["ml1m_shapes"] = shape("ml1m", 6040, 3706, 1_000_000, pick(["ease", "slim", "itemknn", "userknn", "psvd"]),
                                   ns or [64, 1024, 6040], a.reps, a.loop_users, 10)
    if a.only in (None, "ml20m"):
        out["ml20m_shapes"] = shape("ml20m", 138493, 26744, 20_000_000, pick(["psvd", "itemknn", "slim"]),
                                    ns or [64, 4096, fit20, 138493], a.reps, a.loop_users, 0)
    if a.only in (None, "ease20m"):
        out["ml20m_ease_SLICE_of_4096_users"] = shape("ml20m", 138493, 26744, 20_000_000, pick(["ease"]), ns or [64, 4096],
                                                      a.reps, a.loop_users, 0)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
