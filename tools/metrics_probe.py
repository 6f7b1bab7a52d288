#!/usr/bin/env python
"""Times of DESIGN.md §20 (the ranking KPIs) on the device; prints plain lines (kept under profiles/):

    python tools/metrics_probe.py > profiles/metrics_probe.txt

Synthetic lists at n = 1 M users, K = 50, item_num = 100 K, ten truths per user (about 8 % of the positions hit):
  * the one-call KPI pass (`daisy_ranking_kpis`): the default five KPIs at the six cutoffs, the same with int32 lists, and
    all ten per-list KPIs but diversity plus coverage;
  * the diversity pass alone, 19 categories.
Each line: the median of the timed regions (device events) after warm-up, the bytes the pass has to move (lists, owners,
truth rows and row pointers once; tables and partial sums are noise next to them) and that traffic as a fraction of the
6.3 TB/s a copy reaches on this part.  Nothing here is a pass/fail threshold.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from daisyrec_amd import ops  # noqa: E402

DEV = "cuda"
HBM = 6.3e12
DEFAULT = ["recall", "mrr", "ndcg", "hit", "precision"]
CUTOFFS = [1, 5, 10, 20, 30, 50]


def timed(fn, reps=15, warm=3):
    """median milliseconds of fn() between two events"""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main(n=1_000_000, K=50, I=100_000, T=10, C=19):
    print(torch.cuda.get_device_name(0), f"n={n} K={K} item_num={I} truths/user={T}")
    g = torch.Generator(device=DEV).manual_seed(0)
    truths = torch.sort(torch.randint(0, I, (n, T), device=DEV, generator=g), dim=1).values
    indptr = torch.arange(n + 1, device=DEV, dtype=torch.int64) * T
    gt_items = truths.reshape(-1).to(torch.int32).contiguous()
    pred = torch.randint(0, I, (n, K), device=DEV, generator=g)
    plant = torch.rand(n, K, device=DEV, generator=g) < 0.08
    users = torch.randperm(n, device=DEV, generator=g)                  # list r belongs to user users[r]
    pred = torch.where(plant, truths[users][:, torch.randint(0, T, (K,), device=DEV, generator=g)], pred).contiguous()
    disc = torch.from_numpy(1 / np.log2(np.arange(2, K + 2))).to(DEV)
    item_pop = torch.randint(0, 1000, (I,), device=DEV, generator=g).double()
    cats = (np.random.default_rng(0).random((I, C)) < 0.3).astype(np.uint8)
    bits = torch.from_numpy(np.packbits(np.pad(cats, ((0, 0), (0, 64 - C))), axis=1, bitorder="little").view("<u8")
                            .astype(np.int64).reshape(I, 1)).to(DEV)
    sqrt_tab = torch.from_numpy(np.sqrt(np.arange(C + 1))).to(DEV)

    def run(p, metrics):
        return ops.ranking_kpis(p, indptr, gt_items, users, CUTOFFS, metrics, I, disc=disc, item_pop=item_pop, cat_bits=bits,
                                n_cats=C, sqrt_tab=sqrt_tab)

    def line(what, p, metrics, truth_bytes=True):
        moved = p.numel() * p.element_size() + (n * 8 + n * 16 + n * T * 4 if truth_bytes else 0)
        med, lo, hi = timed(lambda: run(p, metrics))
        print(f"{what}: {med:.3f} ms median of 15 (min {lo:.3f}, max {hi:.3f}); {moved / 1e6:.0f} MB to move, "
              f"{moved / (med * 1e-3) / 1e9:.0f} GB/s = {moved / (med * 1e-3) / HBM:.2f} of {HBM / 1e12:.1f} TB/s; "
              f"{med * 1e6 / n:.2f} ns per user")

    names, _, means, _ = run(pred, DEFAULT)
    print("means at the cutoffs", CUTOFFS, {m: [round(float(x), 4) for x in means[s].cpu()] for s, m in enumerate(names)})
    line("KPI pass, default five KPIs x six cutoffs, int64 lists", pred, DEFAULT)
    line("KPI pass, default five KPIs x six cutoffs, int32 lists", pred.to(torch.int32), DEFAULT)
    line("KPI pass, nine per-list KPIs + coverage x six cutoffs, int64 lists", pred,
         ["precision", "recall", "hit", "mrr", "map", "ndcg", "f1", "auc", "popularity", "coverage"])
    line("Diversity pass, 19 categories x six cutoffs, int64 lists", pred, ["diversity"], truth_bytes=False)


if __name__ == "__main__":
    main()
