#!/usr/bin/env python
"""Times of DESIGN.md §28 (ops.{ease,slim,knn,psvd}_full_rank_positions and ops.rank_rows_positions_f32: the exact ranks
of held-out items by counting inside the selectors of §25 and §26) on the device; writes ONE JSON object to
profiles/bench_full_rank_positions_f64.json (or --out):

    python tools/bench_full_rank_positions_f64.py

Shapes and operands are tools/bench_full_rank_f64.py's (§25: ml-1m for the five models, ml-20m for PureSVD, ItemKNN and a
SLiM-like W, EASE at ml-20m on a slice of 4096 users); the exclusion is X's own CSR, the targets are 10 random items per
user.  Per shape and n, in the same process: one *_full_rank_positions call (positions and eligible counts) beside one
*_full_rank_users(topk=50) call, both with validate=False and the output allocation included - device events around the
call, a warm-up call, the median of --reps regions of about 50 ms - and their ratio.  The scored family: one 256 MiB
chunk of N(0, 1) scores, rank_rows_positions_f32 beside rank_rows_f32(topk=50) into preallocated outputs, as the models'
chunk loops call them.  Nothing here is a pass/fail threshold."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from daisyrec_amd import ops  # noqa: E402
from bench_full_rank_f64 import DEV, TOPK, sparse_by_column, timed, zipf_pairs  # noqa: E402

TARGETS_PER_USER = 10
CHUNK_BYTES = 256 << 20


def model_calls(name, U, I, X, Xt, g, factors):
    """(positions(users, targets, exclude), lists(users, exclude)) of a model: bench_full_rank_f64.model_calls' operands"""
    kw = dict(return_eligible=True, validate=False)
    if name == "ease":
        W = torch.randn(I, I, device=DEV, generator=g, dtype=torch.float64)
        return (lambda us, tg, ex: ops.ease_full_rank_positions(X, W, us, tg, exclude=ex, **kw),
                lambda us, ex: ops.ease_full_rank_users(X, W, us, TOPK, exclude=ex, validate=False))
    if name == "psvd":
        uv = torch.randn(U, factors, device=DEV, generator=g, dtype=torch.float64)
        iv = torch.randn(I, factors, device=DEV, generator=g, dtype=torch.float64)
        return (lambda us, tg, ex: ops.psvd_full_rank_positions(uv, iv, us, tg, exclude=ex, **kw),
                lambda us, ex: ops.psvd_full_rank_users(uv, iv, us, TOPK, exclude=ex, validate=False))
    if name == "slim":
        W = sparse_by_column(I, I, 50, g)
        return (lambda us, tg, ex: ops.slim_full_rank_positions(X, W, I, us, tg, exclude=ex, **kw),
                lambda us, ex: ops.slim_full_rank_users(X, W, I, us, TOPK, exclude=ex, validate=False))
    if name == "itemknn":
        W = sparse_by_column(I, I, 40, g)
        return (lambda us, tg, ex: ops.knn_full_rank_positions(X, W, I, I, us, tg, exclude=ex, **kw),
                lambda us, ex: ops.knn_full_rank_users(X, W, I, I, us, TOPK, exclude=ex, validate=False))
    S = sparse_by_column(U, U, 40, g)          # userknn: the similarity's rows (a CSR over users), X by column
    return (lambda us, tg, ex: ops.knn_full_rank_positions(S, Xt, U, I, us, tg, exclude=ex, **kw),
            lambda us, ex: ops.knn_full_rank_users(S, Xt, U, I, us, TOPK, exclude=ex, validate=False))


def rows_chunk(U, I, excl, targets, g, reps):
    """one chunk of CHUNK_BYTES of scores: rank_rows_positions_f32 beside rank_rows_f32(topk), outputs preallocated"""
    rows = max(1, CHUNK_BYTES // (4 * I))
    scores = torch.randn(rows, I, device=DEV, generator=g)
    ru = torch.randint(0, U, (rows,), device=DEV, generator=g)
    out_indptr, pos, el = ops.rank_rows_positions_f32(scores, ru, targets, exclude=excl, return_eligible=True, validate=False)
    ids = torch.empty(rows, TOPK, dtype=torch.int64, device=DEV)
    ms_pos = timed(lambda: ops.rank_rows_positions_f32(scores, ru, targets, exclude=excl, validate=False,
                                                       out=(out_indptr, pos, None, el)), reps)
    ms_list = timed(lambda: ops.rank_rows_f32(scores, TOPK, row_users=ru, exclude=excl, validate=False, out=(ids, None)), reps)
    return {"rows": rows, "items": I, "chunk_bytes": rows * I * 4, "targets": int(pos.numel()), "positions_ms": ms_pos,
            "lists_ms": ms_list, "positions_over_lists": round(ms_pos / ms_list, 3),
            "positions_GB_per_s": round(rows * I * 4 / (ms_pos * 1e-3) / 1e9, 1)}


def shape(tag, U, I, entries, models, ns, reps, seed, factors=150, with_rows=True):
    g = torch.Generator(device=DEV).manual_seed(seed)
    users, items = zipf_pairs(U, I, entries, g)
    ratings = torch.randint(1, 6, (entries,), device=DEV, generator=g).double()
    X = ops.slim_csr(users, items, ratings, U, I)
    Xt = ops.slim_csr(items, users, ratings, I, U) if "userknn" in models else None
    excl = (X[0], X[1])
    t_ptr, t_items, _ = sparse_by_column(I, U, TARGETS_PER_USER, g)      # 10 distinct ascending items per user
    targets = (t_ptr, t_items)
    out = {"users": U, "items": I, "entries": entries, "topk": TOPK, "targets_per_user": TARGETS_PER_USER, "models": {}}
    for name, n_list in models.items():
        positions, lists = model_calls(name, U, I, X, Xt, g, factors)
        rec = []
        for n in (n_list or ns):
            sel = torch.randperm(U, device=DEV, generator=g)[:n].contiguous()
            ms_pos = timed(lambda: positions(sel, targets, excl), reps)
            ms_list = timed(lambda: lists(sel, excl), reps)
            _, pos, el = positions(sel, targets, excl)
            call = {"n": n, "positions_ms": ms_pos, "lists_ms": ms_list, "positions_over_lists": round(ms_pos / ms_list, 3),
                    "targets": int(pos.numel()), "targets_not_ranked": int((pos < 0).sum().item()),
                    "targets_below_topk": int(((pos >= 0) & (pos < TOPK)).sum().item())}
            rec.append(call)
            print(tag, name, json.dumps(call), file=sys.stderr, flush=True)
        out["models"][name] = rec
        del positions, lists
        torch.cuda.empty_cache()
    if with_rows:
        out["rank_rows_one_chunk"] = rows_chunk(U, I, excl, targets, g, reps)
        print(tag, "rank_rows", json.dumps(out["rank_rows_one_chunk"]), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["ml1m", "ml20m", "ease20m"], default=None)
    ap.add_argument("--models", default=None, help="comma-separated subset of the models")
    ap.add_argument("--ns", default=None, help="comma-separated user counts instead of the shape's own")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_full_rank_positions_f64.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_full_rank_positions_f64 needs a HIP device")
    if a.reps < 3:
        raise SystemExit("at least 3 timed regions")
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "region_ms": 50.0, "chunk_bytes": CHUNK_BYTES}
    ns = [int(x) for x in a.ns.split(",")] if a.ns else None
    pick = lambda names: dict.fromkeys(m for m in names if a.models is None or m in a.models.split(","))      # noqa: E731
    if a.only in (None, "ml1m"):
        out["ml1m_shapes"] = shape("ml1m", 6040, 3706, 1_000_000, pick(["ease", "slim", "itemknn", "userknn", "psvd"]),
                                   ns or [64, 1024, 6040], a.reps, 10)
    if a.only in (None, "ml20m"):
        out["ml20m_shapes"] = shape("ml20m", 138493, 26744, 20_000_000, pick(["psvd", "itemknn", "slim"]),
                                    ns or [64, 4096, 138493], a.reps, 0)
    if a.only in (None, "ease20m"):
        out["ml20m_ease_SLICE_of_4096_users"] = shape("ml20m", 138493, 26744, 20_000_000, pick(["ease"]), ns or [64, 4096],
                                                      a.reps, 0, with_rows=False)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
