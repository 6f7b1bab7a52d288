#!/usr/bin/env python
"""Golden lists for the full-ranking protocol, generated from the REAL reference: `MF.full_rank` and
`FM.full_rank` (MFRecommender.py:126-133, FMRecommender.py:125-133) on CPU torch, imported through make_golden; nothing
is copied.  Runs only in the build container; the output tests/golden/kat_full_rank.npz is committed.

    python tests/golden/make_golden_full_rank.py

The tables are EXACT in the sense of tests/full_rank_oracle.py (integers in [-128, 128], FM's biases integers too), so
the reference's fp32 scores are the integer sums whatever order its matmul adds in.  torch.argsort is not stable, so a
tie would not be a fixed answer: before anything is written the script asserts, in integer arithmetic, that no user
has a tie inside the top 11."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (sets up the shims and the reference import path)

import torch  # noqa: E402
import yaml  # noqa: E402
from daisy.model.FMRecommender import FM  # noqa: E402
from daisy.model.MFRecommender import MF  # noqa: E402

U, I, D, TOPK = 40, 333, 16, 10


def main():
    rng = np.random.default_rng(2024)
    P = rng.integers(-128, 129, size=(U, D)).astype(np.float32)
    Q = rng.integers(-128, 129, size=(I, D)).astype(np.float32)
    bu = rng.integers(-50, 51, size=(U, 1)).astype(np.float32)
    bi = rng.integers(-50, 51, size=(I, 1)).astype(np.float32)
    b0 = np.array([7.0], dtype=np.float32)
    s_mf = P.astype(np.int64) @ Q.astype(np.int64).T
    s_fm = s_mf + bu.astype(np.int64) + bi.astype(np.int64).T + int(b0[0])
    for name, s in (("mf", s_mf), ("fm", s_fm)):
        top = -np.sort(-s, axis=1)[:, :TOPK + 1]
        assert np.all(top[:, 1:] < top[:, :-1]), f"{name}: a tie inside the top {TOPK + 1}: draw other tables"
    mf = MF(G.base_config(user_num=U, item_num=I, factors=D, topk=TOPK))
    cfg = G.base_config(user_num=U, item_num=I, factors=D, topk=TOPK)
    cfg.update(yaml.safe_load(open(os.path.join(G.REF, "daisy/assets/fm.yaml"))))
    cfg.update(user_num=U, item_num=I, factors=D, topk=TOPK)
    fm = FM(cfg)
    with torch.no_grad():
        for m in (mf, fm):
            m.embed_user.weight.copy_(torch.from_numpy(P))
            m.embed_item.weight.copy_(torch.from_numpy(Q))
        fm.u_bias.weight.copy_(torch.from_numpy(bu))
        fm.i_bias.weight.copy_(torch.from_numpy(bi))
        fm.bias_.copy_(torch.from_numpy(b0))
    full_mf = np.stack([np.asarray(mf.full_rank(u)) for u in range(U)]).astype(np.int64)
    full_fm = np.stack([np.asarray(fm.full_rank(u)) for u in range(U)]).astype(np.int64)
    assert full_mf.shape == (U, TOPK) and full_fm.shape == (U, TOPK)
    np.savez_compressed(os.path.join(HERE, "kat_full_rank.npz"), P=P, Q=Q, bu=bu, bi=bi, b0=b0, topk=np.int64(TOPK),
                        full_mf=full_mf, full_fm=full_fm)
    print("kat_full_rank.npz: MF", full_mf.shape, "FM", full_fm.shape)


if __name__ == "__main__":
    main()
