#!/usr/bin/env python
"""Times of DESIGN.md §26 (full_rank_users of NeuMF, NFM and VAECF: a bounded score chunk from the model's own score
kernel, then ops.rank_rows_f32) on the device; writes ONE JSON object to profiles/bench_full_rank_scored.json (or --out):

    python tools/bench_full_rank_scored.py

Shapes: ml-1m (6040 x 3706, 1 M exclusion entries) for NeuMF (factors 64, 3 layers, precision 'fp32' and 'bf16') and NFM
(nfm.yaml: 30 factors, 2 layers, relu, batch_norm); ml-20m (138 493 x 26 744, 20 M entries, Zipf users) for VAECF
(multi-vae.yaml: hidden [600], latent_dim 128).  The tables are the models' random initialisation and the interactions
synthetic: fitting is not what is timed.  topk = 50; the exclusion is the interactions' CSR (the training items).
Per shape: the call over ALL users with validate=False at chunk_bytes of 16, 64 and 256 MiB (device events around the
call, a warm-up call, the median of --reps timed regions); the loop it replaces - model.full_rank(u) with its
device-to-host copy, which excludes nothing - timed with the host clock on --loop-users users and EXTRAPOLATED linearly
to all users (marked as such); the selector alone on one 64 MiB chunk of the model's scores next to a device-to-device
copy of the same chunk.  --trace-calls N instead runs N untimed calls at the default chunk and writes nothing: the run to
put under a kernel trace; --kernel-stats tag=CSV adds the per-kernel totals of such a trace to the JSON.  Nothing here is
a pass/fail threshold."""
import argparse
import csv
import json
import logging
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from daisyrec_amd import model as M  # noqa: E402
from daisyrec_amd import ops  # noqa: E402

DEV = "cuda"
REGION_MS = 50.0
TOPK = 50
CHUNKS_MIB = (16, 64, 256)
TAGS = ("neumf_fp32", "neumf_bf16", "nfm", "vae")


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


def pairs(U, I, entries, g, zipf):
    """`entries` distinct (user, item) pairs: users log-uniform over [0, U) (Zipf, exponent 1) or uniform, items uniform"""
    draw = int(entries * 1.4)
    while True:
        if zipf:
            user = (torch.exp(torch.rand(draw, device=DEV, generator=g, dtype=torch.float64) * np.log(U)).to(torch.int64) - 1)
            user = user.clamp_(0, U - 1)
        else:
            user = torch.randint(0, U, (draw,), device=DEV, generator=g)
        item = torch.randint(0, I, (draw,), device=DEV, generator=g)
        key = torch.unique(user * I + item)
        if key.numel() >= entries:
            break
        draw *= 2
    key = key[torch.randperm(key.numel(), device=DEV, generator=g)[:entries]]
    return key // I, key % I


def config(**over):
    cfg = dict(gpu="0", seed=2022, reproducibility=True, topk=TOPK, cand_num=1000, sample_method="uniform", sample_ratio=0,
               num_ng=1, batch_size=256, loss_type="BPR", init_method="default", optimizer="default", early_stop=False,
               UID_NAME="user", IID_NAME="item", INTER_NAME="rating", TID_NAME="timestamp", epochs=1, lr=0.01, reg_1=0.0,
               reg_2=0.0, logger=logging.getLogger("bench"), progress=False)
    cfg.update(over)
    return cfg


def build(tag, U, I, users, items):
    torch.manual_seed(7)
    if tag.startswith("neumf"):
        return M.NeuMF(config(algo_name="neumf", user_num=U, item_num=I, factors=64, num_layers=3, dropout=0.0,
                              model_name="NeuMF", GMF_model=None, MLP_model=None, precision=tag.split("_")[1]))
    if tag == "nfm":
        return M.NFM(config(algo_name="nfm", user_num=U, item_num=I, factors=30, act_function="relu", num_layers=2,
                            batch_norm=True, dropout=0.5)).eval()
    indptr, csr_items = ops.build_user_csr(users.to(torch.int32), items.to(torch.int32), U)
    csr = (indptr, csr_items, torch.ones(csr_items.numel(), dtype=torch.float32, device=DEV))
    return M.VAECF(config(algo_name="multi-vae", user_num=U, item_num=I, mlp_hidden_size=None, latent_dim=128, dropout=0.5,
                          total_anneal_steps=100000, anneal_cap=0.2, history_csr=csr)).eval()


def one_chunk_of_scores(tag, m, I, users):
    """[rows, I] scores of the first 64 MiB chunk of users, from the model's own score entry"""
    rows = min(users.numel(), (64 << 20) // (4 * I))
    us = users[:rows].contiguous()
    buf = torch.empty(rows, I, dtype=torch.float32, device=DEV)
    if tag.startswith("neumf"):
        ctx = m._ctx(min(rows * I, 1 << 18))
        ctx.scores_users(m._params(), us, buf)
        torch.cuda.synchronize()
        ctx.close()
    elif tag == "nfm":
        m._score_ctx(1).scores_users(m._params(), m._bn(), us, buf)
    else:
        buf.copy_(m._scores(us))
    return us, buf


def shape(tag, U, I, entries, zipf, reps, loop_users, trace_calls):
    g = torch.Generator(device=DEV).manual_seed(10)
    users, items = pairs(U, I, entries, g, zipf)
    excl = ops.build_user_csr(users.to(torch.int32), items.to(torch.int32), U)
    m = build(tag, U, I, users, items)
    all_users = torch.randperm(U, device=DEV, generator=g)
    call = lambda mib: m.full_rank_users(all_users, exclude=excl, validate=False,                  # noqa: E731
                                         chunk_bytes=None if mib is None else mib << 20)
    if trace_calls:
        for _ in range(trace_calls + 1):
            call(None)
        torch.cuda.synchronize()
        return None
    out = {"users": U, "items": I, "exclusion_entries": entries, "topk": TOPK, "n": U}
    ids = call(None)
    assert ids.shape == (U, TOPK)
    out["lists_with_fewer_eligible_items"] = int((ids[:, -1] < 0).sum().item())
    out["call_ms_by_chunk_MiB"] = {str(mib): timed(lambda: call(mib), reps) for mib in CHUNKS_MIB}
    out["call_ms_without_exclusion_default_chunk"] = timed(lambda: m.full_rank_users(all_users, validate=False), reps)
    # the loop this replaces: the parent's code path, one user at a time, nothing excluded
    singles = [int(u) for u in all_users[:min(loop_users, U)].tolist()]
    for u in singles[:20]:
        m.full_rank(u)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for u in singles:
        m.full_rank(u)
    loop_ms = (time.perf_counter() - t0) * 1e3 / len(singles)
    out["loop_full_rank_users_timed"] = len(singles)
    out["loop_full_rank_ms_per_user"] = round(loop_ms, 4)
    out["loop_full_rank_ms_EXTRAPOLATED"] = round(loop_ms * U, 1)
    # the selector alone on one chunk, next to a device-to-device copy of that chunk in the same process
    us, buf = one_chunk_of_scores(tag, m, I, all_users)
    dst = torch.empty_like(buf)
    sel_ms = timed(lambda: ops.rank_rows_f32(buf, TOPK, row_users=us, exclude=excl, validate=False), reps)
    sel0_ms = timed(lambda: ops.rank_rows_f32(buf, TOPK), reps)
    copy_ms = timed(lambda: dst.copy_(buf), reps)
    nbytes = buf.numel() * 4
    out["selector_one_chunk"] = {"rows": int(buf.shape[0]), "score_bytes": nbytes, "ms": sel_ms, "ms_without_exclusion": sel0_ms,
                                 "score_GB_read_per_s": round(nbytes / (sel_ms * 1e-3) / 1e9, 1),
                                 "d2d_copy_ms": copy_ms,
                                 "d2d_copy_GB_copied_per_s": round(nbytes / (copy_ms * 1e-3) / 1e9, 1),
                                 "note": "a copy reads and writes every byte, the selector only reads"}
    best = min(out["call_ms_by_chunk_MiB"].values())
    out["ratio_loop_EXTRAPOLATED_to_best_call"] = round(out["loop_full_rank_ms_EXTRAPOLATED"] / best, 1)
    print(tag, json.dumps(out), file=sys.stderr, flush=True)
    return out


def kernel_split(path):
    """per-kernel totals of a rocprofv3 --kernel-trace --stats CSV: the selector against everything else of the run"""
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    sel = sum(float(r["TotalDurationNs"]) for r in rows if "k_rank_rows_f32" in r["Name"])
    top = sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:8]
    return {"kernel_ms_total": round(total / 1e6, 3), "k_rank_rows_f32_ms": round(sel / 1e6, 3),
            "selector_share": round(sel / total, 4) if total else None,
            "largest_kernels": [{"name": r["Name"][:90], "calls": int(r["Calls"]), "ms": round(float(r["TotalDurationNs"]) / 1e6, 3)}
                                for r in top]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-users", type=int, default=1000)
    ap.add_argument("--only", default=None, help="comma-separated subset of " + ",".join(TAGS))
    ap.add_argument("--trace-calls", type=int, default=0, help="run this many untimed calls per model and write nothing")
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="TAG=CSV",
                    help="a rocprofv3 kernel stats CSV of a --trace-calls run of one model")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_full_rank_scored.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_full_rank_scored needs a HIP device")
    if not a.trace_calls and (a.reps < 3 or a.loop_users < 1000):
        raise SystemExit("at least 3 timed regions and 1000 loop users")
    tags = a.only.split(",") if a.only else list(TAGS)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "default_chunk_bytes": M.AbstractRecommender.SCORED_CHUNK_BYTES,
           "models": {}}
    for tag in tags:
        big = tag == "vae"
        rec = shape(tag, 138493 if big else 6040, 26744 if big else 3706, 20_000_000 if big else 1_000_000, big, a.reps,
                    a.loop_users, a.trace_calls)
        if rec is not None:
            out["models"][tag] = rec
        torch.cuda.empty_cache()
    if a.trace_calls:
        return
    for item in a.kernel_stats:
        tag, path = item.split("=", 1)
        out["models"].setdefault(tag, {})["kernel_trace"] = kernel_split(path)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
