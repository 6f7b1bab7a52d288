#!/usr/bin/env python
"""Times of DESIGN.md §27 (ops.full_rank_positions: exact ranks of held-out items over all items, and the KPI call on
them) on the device, beside ops.full_rank_users measured IN THE SAME PROCESS; writes ONE JSON object to
profiles/bench_full_rank_positions.json (or --out):

    python tools/bench_full_rank_positions.py

Shapes and method are tools/bench_full_rank.py's: d = 64, I = 26 744, n in {64, 4096, 138 493} of U = 138 493 users with
a Zipf exclusion CSR of 20 M entries, and n = U = 6040, I = 3706 with 1 M entries; tables N(0, 0.1); device events
around the call, a warm-up call, the median of --reps timed regions; validate=False.  The target CSR holds 10 random
items per user (fewer where two draws met), wherever they fall - a few lie inside the exclusion and come out as -1.
Per n: the positions call (eligible counts included, the torch prefix sum of the row lengths and its read-back
included), the same call without the exclusion, the KPI call at 7 cutoffs x 9 KPIs, and full_rank_users at topk 1, 50
and 128 with and without the exclusion.  On random tables a target is as likely anywhere in the order, so most scores
lie ABOVE a user's lowest target and take the counting loop: a trained model's targets sit higher and skip more.

    rocprofv3 --kernel-trace --stats -d DIR -o frp -- python tools/bench_full_rank_positions.py --trace-calls 6

runs six positions + KPI calls at n = U = 138 493 and nothing else (the kernel split of
profiles/full_rank_positions_rocprof_kernel_summary.txt).  Nothing here is a pass/fail threshold."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_full_rank import DEV, MFMA_F32_PEAK, timed, zipf_csr  # noqa: E402
from daisyrec_amd import ops  # noqa: E402

CUTOFFS = [1, 5, 10, 20, 50, 200, 1000]
KPIS = list(ops.POSITION_KPIS)


def target_csr(U, I, per_user, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    user = torch.arange(U, device=DEV).repeat_interleave(per_user)
    item = torch.randint(0, I, (U * per_user,), device=DEV, generator=g)
    key = torch.unique(user * I + item)
    return ops.build_user_csr((key // I).to(torch.int32), (key % I).to(torch.int32), U)


def kpi_call(out_indptr, pos, eligible):
    from daisyrec_amd.utils import metrics as M
    return M.position_kpis(out_indptr, pos, None, eligible, CUTOFFS, KPIS)


def setup(U, I, d, entries, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    P = torch.randn(U, d, device=DEV, generator=g) * 0.1
    Q = torch.randn(I, d, device=DEV, generator=g) * 0.1
    excl, longest = zipf_csr(U, I, entries, seed + 1)
    return P, Q, excl, longest, target_csr(U, I, 10, seed + 2), g


def shape(U, I, d, ns, entries, reps, seed):
    P, Q, excl, longest, targets, g = setup(U, I, d, entries, seed)
    out = {"users": U, "items": I, "d": d, "exclusion_entries": int(excl[1].numel()), "longest_exclusion_row": longest,
           "target_entries": int(targets[1].numel()), "kpi_cutoffs": CUTOFFS, "kpis": KPIS, "calls": []}
    for n in ns:
        users = torch.randperm(U, device=DEV, generator=g)[:n].contiguous()
        run = lambda ex=excl: ops.full_rank_positions(P, Q, users, targets, exclude=ex, return_eligible=True,       # noqa: E731
                                                      validate=False)
        lists = lambda k, ex=excl: ops.full_rank_users(P, Q, users, k, exclude=ex, validate=False)                  # noqa: E731
        ms = timed(run, reps)
        oi, pos, el = run()
        call = {"n": n, "targets": int(pos.numel()), "targets_not_ranked": int((pos < 0).sum().item()),
                "positions_ms": ms, "mfma_fraction": round(2.0 * n * I * d / (ms * 1e-3) / MFMA_F32_PEAK, 4),
                "workspace_bytes": int(ops.lib.daisy_full_rank_positions_workspace_bytes(n, pos.numel())),
                "positions_ms_without_exclusion": timed(lambda: run(ex=None), reps),
                "kpis_ms": timed(lambda: kpi_call(oi, pos, el), reps)}
        for k in (1, 50, 128):
            call[f"full_rank_users_ms_topk_{k}"] = timed(lambda: lists(k), reps)
            call[f"full_rank_users_ms_topk_{k}_without_exclusion"] = timed(lambda: lists(k, None), reps)
        call["positions_over_topk_1"] = round(ms / call["full_rank_users_ms_topk_1"], 3)
        out["calls"].append(call)
        print(json.dumps(call), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace-calls", type=int, default=0, help="only this many positions + KPI calls at the ml-20m shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_full_rank_positions.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_full_rank_positions needs a HIP device")
    if a.trace_calls:
        U, I = 138493, 26744
        P, Q, excl, _, targets, _ = setup(U, I, 64, 20_000_000, 0)
        users = torch.arange(U, device=DEV)
        for _ in range(a.trace_calls):
            oi, pos, el = ops.full_rank_positions(P, Q, users, targets, exclude=excl, return_eligible=True, validate=False)
            kpi_call(oi, pos, el)
        torch.cuda.synchronize()
        return
    if a.reps < 3:
        raise SystemExit("at least 3 timed regions")
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "mfma_f32_peak_flops": MFMA_F32_PEAK,
           "ml20m_shapes": shape(138493, 26744, 64, [64, 4096, 138493], 20_000_000, a.reps, 0),
           "ml1m_shapes": shape(6040, 3706, 64, [6040], 1_000_000, a.reps, 10)}
    with open(a.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
