"""The two kernels on the fp32 MFMA tile stream (tile and helpers: csrc/rank_tiles_f32.h) against each other on inexact
data: the list of ops.full_rank_users (csrc/rank_full.hip) and the positions of ops.full_rank_positions
(csrc/rank_positions.hip) must come from the same scores, masks and sort words, so on Gaussian tables - where no oracle has the bits - a target sits at
position p of the list exactly when p is its position, with the same score bits.  Everything by equality."""
import numpy as np
import pytest
import torch

from test_gpu_full_rank_users import _csr, _random_rows, _t

pytestmark = pytest.mark.gpu
TOPK = 128
N_TARGETS = 40                                          # two slots of 32 per request


# d: one k chunk, four chunks with a tail, nine chunks with a tail (element-by-element rows), and 64 = four whole chunks
# of float4 rows; I, n: three item tiles with two or three user tiles, and just past one item tile with one user tile
@pytest.mark.parametrize("d,I,n,slices,with_biases", [(3, 333, 65, 3, False), (50, 333, 130, 7, True),
                                                      (130, 129, 64, 2, False), (64, 333, 65, 0, False)])
def test_list_and_positions_agree(d, I, n, slices, with_biases):
    from daisyrec_amd import ops
    rng = np.random.default_rng(d * 1000 + I + n)
    U = n + 5
    P = rng.standard_normal((U, d)).astype(np.float32)
    Q = rng.standard_normal((I, d)).astype(np.float32)
    users = rng.integers(0, U, size=n)                  # any order, duplicates
    excl = _csr(_random_rows(rng, U, I), U)
    tgt = _csr({u: sorted(rng.choice(I, size=N_TARGETS, replace=False).tolist()) for u in range(U)}, U)
    biases = None
    if with_biases:
        biases = tuple(_t(rng.standard_normal(s).astype(np.float32)) for s in ((U, 1), (I, 1), (1,)))
    Pd, Qd, ud = _t(P), _t(Q), _t(users.astype(np.int64))
    ex = tuple(_t(x) for x in excl)
    ids, scores = ops.full_rank_users(Pd, Qd, ud, TOPK, exclude=ex, biases=biases, return_scores=True, item_slices=slices)
    out_indptr, pos, tscores, eligible = ops.full_rank_positions(
        Pd, Qd, ud, tuple(_t(x) for x in tgt), exclude=ex, biases=biases, return_scores=True, return_eligible=True,
        item_slices=slices)
    ids, scores = ids.cpu().numpy(), scores.cpu().numpy().view(np.uint32)
    out_indptr, pos, tscores = out_indptr.cpu().numpy(), pos.cpu().numpy(), tscores.cpu().numpy().view(np.uint32)
    eligible = eligible.cpu().numpy()
    assert ids.shape == (n, TOPK) and out_indptr.tolist() == (np.arange(n + 1) * N_TARGETS).tolist()
    seen = {"listed": 0, "beyond": 0, "excluded": 0}
    for b, u in enumerate(users.tolist()):
        row = set(excl[1][excl[0][u]:excl[0][u + 1]].tolist())
        assert eligible[b] == I - len([i for i in row if 0 <= i < I]), (b, u)
        listed = ids[b].tolist()
        for x, t in enumerate(tgt[1][tgt[0][u]:tgt[0][u + 1]].tolist()):
            p = int(pos[out_indptr[b] + x])
            if t in row:
                assert p == -1 and t not in listed, (b, u, t, p)
                seen["excluded"] += 1
            elif p < TOPK:
                assert p >= 0 and listed[p] == t, (b, u, t, p, listed[max(p, 0)])
                assert scores[b, p] == tscores[out_indptr[b] + x], (b, u, t, p)
                seen["listed"] += 1
            else:
                assert t not in listed, (b, u, t, p)
                seen["beyond"] += 1
    assert seen["listed"] and seen["excluded"] and (seen["beyond"] or I - 1 <= TOPK), seen
