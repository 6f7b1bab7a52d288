#!/usr/bin/env python
"""Epoch time of T small-batch MF models trained side by side (ops.fit_epoch_sgd_many: what model.fit_many issues per
epoch) against T stand-alone epochs one after another (what T calls of MF.fit issue), at ml-100k-like sizes:
U = 943, I = 1682, 400 000 triples, B = 256, d in {32, 64, 100}, SGD, BPR, device shuffle.

One "epoch" is what fit_many does between two epochs' bookkeeping: build the plans, zero the accumulators, one native
call over all models, one read-back of all epoch losses - wall time up to the end of that read-back, median of 5 after
one warm-up epoch.  With plan sharing all T models read ONE plan (a grid over lr / reg on one training set); without,
every model builds its own (folds, seeds).  The stand-alone loop is timed for min(T, 4) models and scaled to T (marked
"extrapolated"): its epochs are independent and serial, a model more adds the same time again.

    python tools/bench_fit_many.py [--out profiles/bench_fit_many.json] [--trials 1,4,16,64,256,512] [--factors 32,64,100]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from daisyrec_amd import ops  # noqa: E402
from daisyrec_amd.model.MFRecommender import padded_factors  # noqa: E402

U, I, N, B = 943, 1682, 400_000, 256
UNSHARED_MAX = 64           # a plan of 400 000 triples per model: beyond this the builds alone take the epoch
DEV = "cuda"


def median_of(f, reps=5):
    f()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "bench_fit_many.json"))
    ap.add_argument("--trials", default="1,4,16,64,256,512")
    ap.add_argument("--factors", default="32,64,100")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fit_many needs a HIP device"
    g = torch.Generator().manual_seed(0)
    tri = torch.stack([torch.sort(torch.randint(0, U, (N,), generator=g)).values, torch.randint(0, I, (N,), generator=g),
                       torch.randint(0, I, (N,), generator=g)], 1).to(torch.int32).to(DEV)
    nb = (N + B - 1) // B
    out = {"shape": {"users": U, "items": I, "triples": N, "batch": B, "steps_per_epoch": nb, "optimizer": "sgd", "loss": "BPR",
                     "order": "feistel"},
           "device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
           "metric": "wall seconds of one epoch (plan builds + one native call + one read-back), median of 5", "points": []}
    trial_counts = [int(x) for x in a.trials.split(",")]
    for d in (int(x) for x in a.factors.split(",")):
        dt = padded_factors(d, "auto", B)          # the columns MF trains on at this batch size (d = 100 -> 128)
        Tmax = max(trial_counts)
        tables = [(torch.randn(U, dt, device=DEV) * 0.01, torch.randn(I, dt, device=DEV) * 0.01)
                  for _ in range(Tmax)]
        ctxs = [ops.BprContext(B, dt, U, I, device=DEV) for _ in range(Tmax)]
        plans = [ops.EpochPlan(N, U, I, device=DEV) for _ in range(min(Tmax, UNSHARED_MAX))]
        epoch_no = [0]

        def build(k):
            plans[k].build(tri, B, order="feistel", seed=7 + k, epoch=epoch_no[0], user_sorted=True, validate=False)

        def many_epoch(T, shared):
            epoch_no[0] += 1
            for k in range(1 if shared else T):
                build(k)
            accs = [c.epoch_acc for c in ctxs[:T]]
            torch._foreach_zero_(accs)
            ops.fit_epoch_sgd_many([(ctxs[k], plans[0 if shared else k], tables[k][0], tables[k][1], 0.01 + 1e-5 * k, 1e-3, 1e-3,
                                     ops.N.LOSS_BPR, 1e-10) for k in range(T)])
            return torch.stack(accs).cpu()

        def alone_epochs(T):
            epoch_no[0] += 1
            for k in range(T):
                build(0)
                ctxs[k].epoch_acc.zero_()
                ctxs[k].fit_epoch_sgd(plans[0], tables[k][0], tables[k][1], 0.01 + 1e-5 * k, 1e-3, 1e-3)
                ctxs[k].epoch_acc.cpu()

        def builds_only(count):
            epoch_no[0] += 1
            for k in range(count):
                build(k)

        t_build1 = median_of(lambda: builds_only(1))[0]
        for T in trial_counts:
            Ta = min(T, 4)
            t_alone = median_of(lambda: alone_epochs(Ta))[0]
            point = {"factors": d, "trained_columns": dt, "models": T,
                     "loop_of_fit_epochs": {"seconds": t_alone * T / Ta, "timed_models": Ta, "extrapolated": T > Ta}}
            for shared in (True, False):
                if not shared and T > len(plans):
                    point["own_plans"] = "not measured (a plan per model beyond %d models)" % UNSHARED_MAX
                    continue
                med, lo, hi = median_of(lambda: many_epoch(T, shared))
                t_b = t_build1 if shared else median_of(lambda: builds_only(T))[0]
                point["shared_plan" if shared else "own_plans"] = {
                    "seconds": med, "min": lo, "max": hi, "model_steps_per_s": T * nb / med, "plan_build_seconds": t_b,
                    "plan_build_share": t_b / med, "speedup_over_loop": (t_alone * T / Ta) / med}
            assert float(many_epoch(T, True)[:, 1].sum()) == 0.0, "a step's loss was not finite: the epochs timed were cut short"
            out["points"].append(point)
            print(json.dumps(point), flush=True)
        torch.cuda.synchronize()
        for x in ctxs + plans:
            x.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
