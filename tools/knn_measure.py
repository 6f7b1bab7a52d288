#!/usr/bin/env python
"""Measurements of DESIGN.md §19 (ItemKNN / UserKNN) on the device; prints plain lines (kept under profiles/):

    python tools/knn_measure.py > profiles/knn_measure.txt

  * ItemKNNCF.fit and UserKNNCF.fit at ml-100k's shape (943 x 1682, the synthetic set of
    tests/golden/make_golden_ease.py::time_ml100k), cosine, shrink 100, maxk 40: wall time, best of 3;
  * daisy_knn_select alone at n = 1682 and at a synthetic n = 16384, K = 40, cosine, next to a device-to-device copy of G
    (n^2 x 4 bytes) timed in the same process;
  * daisy_knn_rank for 943 users x all items next to daisy_ease_rank on the same shape.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from daisyrec_amd import ops  # noqa: E402
from daisyrec_amd.model import ItemKNNCF, UserKNNCF  # noqa: E402

DEV = "cuda"


def ml100k_frame():
    import pandas as pd
    rng = np.random.RandomState(0)
    U, I, n = 943, 1682, 100000
    pop = rng.zipf(1.3, I).clip(1, 50).astype(float)
    key = np.unique(rng.randint(0, U, 3 * n).astype(np.int64) * I + rng.choice(I, 3 * n, p=pop / pop.sum()))
    key = rng.permutation(key)[:n]
    return U, I, pd.DataFrame({"user": key // I, "item": key % I, "rating": rng.randint(1, 6, len(key)).astype(float)})


def timed(fn, reps=20, warm=3):
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
    return float(np.median(out))


def whole_fits():
    import logging
    U, I, df = ml100k_frame()
    cfg = dict(maxk=40, shrink=100, normalize=True, similarity="cosine", topk=50, user_num=U, item_num=I, gpu="0",
               logger=logging.getLogger("knn"), UID_NAME="user", IID_NAME="item", INTER_NAME="rating")
    models = {}
    for cls in (ItemKNNCF, UserKNNCF):
        best = np.inf
        for _ in range(4):                                   # the first fit also loads the kernels
            m = cls(dict(cfg))
            torch.cuda.synchronize()
            t0 = time.time()
            m.fit(df)
            torch.cuda.synchronize()
            best = min(best, time.time() - t0)
        models[cls.__name__] = m
        print(f"{cls.__name__}.fit, {U} x {I}, {len(df)} ratings, cosine, shrink 100, maxk 40: {best * 1e3:.1f} ms wall "
              f"(best of 4), nnz(W) {m.fit_info['nnz']}, bytes_peak {m.fit_info['bytes_peak']}")
    return models


def select_alone(n, K=40):
    rng = torch.Generator(device=DEV).manual_seed(n)
    A = (torch.rand(512, n, device=DEV, generator=rng) < 0.06).float() * torch.randint(1, 6, (512, n), device=DEV,
                                                                                       generator=rng).float()
    G = (A.T @ A).contiguous()
    ss = ops.knn_diag(G, True)
    G2 = torch.empty_like(G)
    t_copy = timed(lambda: G2.copy_(G))
    t_sel = timed(lambda: ops.knn_select(G, ss, "cosine", 100.0, K))
    gb = n * n * 4 / 1e9
    print(f"knn_select n={n} K={K} cosine: {t_sel:.3f} ms; device-to-device copy of G ({gb * 1e3:.1f} MB): {t_copy:.3f} ms "
          f"({2 * gb / (t_copy * 1e-3):.0f} GB/s read + write); ratio {t_sel / t_copy:.2f}; five reads of G at "
          f"{5 * gb / (t_sel * 1e-3):.0f} GB/s")


def rank_alone(models):
    m = models["ItemKNNCF"]
    U, I = m.user_num, m.item_num
    users = torch.arange(U, device=DEV)
    t_knn = timed(lambda: ops.knn_rank(m._L, m._R, I, I, users, None, 50))
    t_knn0 = timed(lambda: ops.knn_rank(m._L, m._R, I, I, users, None, 0))
    mu = models["UserKNNCF"]
    t_user = timed(lambda: ops.knn_rank(mu._L, mu._R, U, I, users, None, 50))
    W = torch.randn(I, I, dtype=torch.float64, device=DEV)
    t_ease = timed(lambda: ops.ease_rank(m._csr, W, users, None, 50))
    t_ease0 = timed(lambda: ops.ease_rank(m._csr, W, users, None, 0))
    print(f"rank {U} users x {I} items, topk 50: knn_rank (ItemKNN operands) {t_knn:.3f} ms (scores only {t_knn0:.3f}), "
          f"knn_rank (UserKNN operands) {t_user:.3f} ms, ease_rank {t_ease:.3f} ms (scores only {t_ease0:.3f})")


if __name__ == "__main__":
    print(torch.cuda.get_device_name(0))
    models = whole_fits()
    select_alone(1682)
    select_alone(16384)
    rank_alone(models)
