"""Multi-VAE on the device at the shapes the KATs and the ml-100k replay never reach (tests/vae_cases.py): one training
step of every case through daisy_vae_step_grads against the float64 oracle, twice for the bits, and eval-mode scores of
the scalar first layer.  What each case exists for, in csrc/vae.hip:

  scalar_6, scalar_deep_odd, scalar_1   `v4 ? k_vae_enc0_v4 : k_vae_enc0` in vae_forward and `v4 ? k_vae_w0grad_v4 :
                    k_vae_w0grad` in vae_step with enc[1] % 4 != 0: the scalar kernels (widths 6, 3, 1)
  nohidden_*        `n > 0 ? 1 : 0`, the act argument of k_vae_enc0(_v4): no tanh, the sparse layer feeds k_vae_reparam,
                    `for (int k = 0; k < n; ++k)` of the decoder is empty (lat 6: scalar, lat 8: _v4)
  wide_scalar       `for (int c0 = 0; c0 < d1; c0 += kBlock * kVaeCols)` of k_vae_enc0 / k_vae_w0grad: a second pass
                    with a ragged tail of 3 columns
  wide_v4           `for (int c0 = 0; c0 < d1; c0 += kVaeV4Cols)` of the _v4 kernels: a second pass of one float4, the
                    LDS `red` array reused straight after vae_wave_sum_v4
  runs_*            `per = (B + kBlock - 1) / kBlock` > 1 in k_vae_offsets and k_vae_loss; `if (n < kBlock) break` of
                    k_vae_w0grad(_v4) with item runs of 300, exactly 256 (the next tile matches nothing), 257, and a
                    last run of 256 whose next tile starts at `qq == E`; `if (cf == 0.f) continue` inside them; the
                    `b == a.B - 1` padding branch of k_vae_prep with an empty last row; runs_ratings: values 1..5
                    through `v / denom`, `rsum`, `ent_val` in k_vae_softmax
  rows_*            `for (int e0 = 0; e0 < len; e0 += kBlock)` of k_vae_enc0(_v4) with rows of 256, 257, 512, 513, 3
                    and 0 entries: full last tiles
  hot_softmax       `if (v > m)` and the `(m, s)` tree of k_vae_softmax, `lse = smm[0] + logf(sms[0])`, `expf(zr[i] +
                    bias[i] - lse)`: logits of -100 .. 100, expf(100) overflows fp32

Bounds (test_step_gradients_against_oracle): loss 1e-5 relative, every gradient within 1e-5 of the oracle
tensor's largest element; tests/test_oracle_vae.py holds the reference's own fp32 arithmetic to the same bounds."""
import numpy as np
import pytest
import torch

import vae_cases as VC
from test_gpu_vae import f32, grad_views, host_state
from test_oracle_vae import vae_config

pytestmark = pytest.mark.gpu


def case_model(c):
    """VAECF with the case's widths and histories (user b is row b of R), the case's state loaded"""
    from daisyrec_amd.model import VAECF
    torch.manual_seed(0)
    m = VAECF(vae_config(user_num=c.B, item_num=c.I, mlp_hidden_size=list(c.hidden), latent_dim=c.lat, dropout=c.p,
                         history_item_id=torch.from_numpy(c.hist_id.copy()),
                         history_item_value=torch.from_numpy(c.hist_val.copy())))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in c.state.items()})
    return m


@pytest.mark.parametrize("name", VC.NAMES)
def test_edge_step_against_oracle_and_bitwise_repeat(name):
    from daisyrec_amd import ops
    from daisyrec_amd import _native as N
    c = VC.case(name)
    m = case_model(c)
    init = host_state(m)
    assert all(np.array_equal(init[k], c.state[k]) for k in c.state)
    W = m._params()
    csr, lens = m._csr()
    E = int(lens.sum())
    assert E == c.keep.size and m.layers == c.hidden                   # n_entries exact: no sentinel after the last run
    assert W.data_ptr() % 16 == 0                                      # the form is chosen by the width alone
    users = torch.arange(c.B, dtype=torch.int64).cuda()
    keep, eps = torch.from_numpy(c.keep.copy()).cuda(), torch.from_numpy(c.eps.copy()).cuda()
    ctx = ops.VaeContext(c.B, max(E, 1), c.I, m.layers, c.lat)
    try:
        assert ctx.param_count == W.numel()
        out = []
        for _ in range(2):
            g = torch.zeros_like(W)
            assert g.data_ptr() % 16 == 0
            ctx.stats.zero_()
            ctx.step_grads(W, g, csr, users, E, keep=keep, eps=eps, train=True, dropout=c.p, anneal=f32(c.anneal))
            stats = ctx.stats.cpu().numpy().copy()
            out.append((stats, g.cpu().numpy().copy(), grad_views(m, g)))
    finally:
        ctx.close()
    (stats, flat, grads), (stats2, flat2, _) = out
    loss = float(stats[N.VST_LOSS])
    lerr, gerr = VC.errors(loss, grads, name)
    print(name, "device step: loss error", lerr, "worst gradient error", max(gerr.values()), "in",
          max(gerr, key=gerr.get))
    assert np.isfinite(flat).all(), name
    assert stats[N.VST_BAD_ROWS] == 0 and stats[N.VST_NONFINITE] == 0
    assert lerr <= 1e-5, (name, loss, lerr)
    for k, e in gerr.items():
        assert e <= 1e-5, (name, k, e)
    # fixed-order sums: the same bits from the same inputs
    assert np.array_equal(flat.view(np.uint32), flat2.view(np.uint32)), name
    assert np.array_equal(stats[[N.VST_LOSS]].view(np.uint64), stats2[[N.VST_LOSS]].view(np.uint64)), name


@pytest.mark.parametrize("name", ["scalar_6", "nohidden_scalar", "rows_scalar"])
def test_edge_eval_scores_through_the_scalar_first_layer(name):
    """daisy_vae_scores -> vae_forward with train = 0 -> k_vae_enc0 (scalar: the width is no multiple of 4), where the
    coefficients are the normalised values themselves: all items (the output GEMM) and a [B, 5] candidate block
    (k_vae_gather_scores) against the oracle's eval-mode forward, at the tolerance
    test_rank_full_rank_predict_against_reference applies to scores (rtol 1e-5, atol 1e-6)."""
    from daisyrec_amd import ops
    c = VC.case(name)
    assert (c.hidden + [c.lat])[0] % 4 != 0
    m = case_model(c)
    W = m._params()
    csr, lens = m._csr()
    E = int(lens.sum())
    users = torch.arange(c.B, dtype=torch.int64).cuda()
    ref = VC.eval_scores(name)
    cands = np.random.default_rng(VC.SEEDS[name]).integers(0, c.I, size=(c.B, 5))
    ctx = ops.VaeContext(c.B, max(E, 1), c.I, m.layers, c.lat)
    try:
        full = ctx.scores(W, csr, users, E).cpu().numpy()
        some = ctx.scores(W, csr, users, E, items=torch.from_numpy(cands).cuda()).cpu().numpy()
    finally:
        ctx.close()
    print(name, "eval scores: worst absolute error", np.abs(full - ref).max(), "of scores up to", np.abs(ref).max())
    np.testing.assert_allclose(full, ref, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(some, np.take_along_axis(ref, cands, axis=1), rtol=1e-5, atol=1e-6)
