"""Shared inputs of tests/test_gpu_fit_many.py and tests/test_host_fit_many.py.

Sizes.  U = 40 users, I = 30 items, n = 600 random triples: two full batches of 256 and one of 88, every user about six
times and every item about seventeen times in a full batch (runs of equal ids on both sides of a step).

The exact set.  `exact_cases()` draws models from the exact domain of tests/segment_layouts.py - tables of integers in
{-1, 0, 1}, reg_1 = reg_2 = 0, the hinge loss and a power-of-two learning rate - and chains `segment_layouts.exact_step`
over the batches of one identity-order epoch.  The learning rate is 2^0: the updated tables are integers again, which
`exact_step` needs of its input, so the chain stays in int64 from the first step to the last; `assert_exact_domain` is
checked on every step of the chain (the host test does that without a device), so whatever order a kernel adds a row's
terms in, its fp32 sums are the integers of the chain (after three steps the largest table element is about 60).
"""
import numpy as np
import torch

import segment_layouts as S

U, I, N_TRIPLES = 40, 30, 600
EXACT_B, EXACT_LR = 256, 1.0
EXACT_D = ((32, "auto"), (64, "auto"), (20, 0))          # (factors, row_pitch): exact lanes twice, masked lanes once


def triples(n=N_TRIPLES, users=U, items=I, seed=11):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, users, n), rng.integers(0, items, n), rng.integers(0, items, n)], 1).astype(np.int32)


class ExactCase:
    """one model of the exact set: its start tables, and after `chain()` the int64 tables and the loss of the epoch"""

    def __init__(self, d, pitch, seed):
        rng = np.random.default_rng(seed)
        self.d, self.pitch = d, pitch
        self.P0 = rng.integers(-1, 2, (U, d)).astype(np.float32)
        self.Q0 = rng.integers(-1, 2, (I, d)).astype(np.float32)

    def chain(self, tri, device="cpu"):
        """exact_step over the batches of the identity-order epoch of `tri`; every step is checked to be in the domain"""
        P = torch.from_numpy(self.P0).to(torch.int64).to(device)
        Q = torch.from_numpy(self.Q0).to(torch.int64).to(device)
        loss = 0
        for lo in range(0, len(tri), EXACT_B):
            b = tri[lo:lo + EXACT_B].astype(np.int64)
            st = S.exact_step(P, Q, b[:, 0], b[:, 1], b[:, 2], S.HL, EXACT_LR, device=device)
            S.assert_exact_domain(st)
            P = P.clone().index_add_(0, st.urows, -st.gP)          # lr = 1: the update in integers
            Q = Q.clone().index_add_(0, st.irows, -st.gQ)
            assert torch.equal(P.to(torch.float32), st.P_new()) and torch.equal(Q.to(torch.float32), st.Q_new())
            loss += st.loss
        self.P, self.Q, self.loss = P, Q, loss
        return self


def exact_cases():
    return [ExactCase(d, pitch, 100 + k) for k, (d, pitch) in enumerate(EXACT_D)]
