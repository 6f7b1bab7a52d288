"""NFM on the GPU: the kernels of csrc/nfm.hip through the mirror class against the REAL reference NFM's golden vectors
(tests/golden/kat_nfm.npz) and against the float64 oracle (tests/nfm_oracle.py, gradients by torch autograd)."""
import os

import numpy as np
import pytest
import torch

import nfm_oracle as NO
from test_oracle_nfm import close, kat_model, nfm_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["nf_bpr_sgd", "nf_bpr_sgd_nobn", "nf_bpr_adam_reg", "nf_hl_sgd_reg", "nf_tl_adam", "nf_cl_sgd_reg", "nf_cl_adam",
         "nf_sl_sgd", "nf_sl_adam_reg_nobn", "nf_bpr_adam_L0_nobn", "nf_hl_adam_other"]


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(HERE, "golden", "kat_nfm.npz"))


def _np(t):
    return t.detach().cpu().numpy()


def _i32(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(torch.int32).to(DEV)


def _steps(model, triples, seed_steps=None):
    """calc_loss + backward + optimizer.step of the reference per (u, i, j), on the library's kernels."""
    from daisyrec_amd import ops
    from daisyrec_amd import _native as N
    p = model._params()
    loss_id = ops.LOSS_IDS[model.loss_type.upper()]
    optim = ops.DenseOptimizer(model._resolve_optimizer(), model.lr)
    gflat = torch.zeros_like(model._flat)
    g = model._grad_table(gflat)
    ctx = model._ctx(max(len(t[0]) for t in triples))
    losses = []
    try:
        for k, (u, i, j) in enumerate(triples):
            ctx.step_grads(p, g, model._bn(), _i32(u), _i32(i), _i32(j), loss_id, model.reg_1, model.reg_2,
                           dropout=model.dropout, seed=seed_steps[k] if seed_steps else k + 1)
            losses.append(float(ctx.stats[N.NFST_LOSS].cpu()))
            optim.next_step()
            optim.step(model._flat, gflat)
    finally:
        ctx.close()
    return losses


@pytest.mark.parametrize("path", ["small", "layered"])
@pytest.mark.parametrize("case", CASES)
def test_step_kats_against_the_reference(kat, case, path):
    U, I, f, L, bn, B, ns, seed = (int(x) for x in kat[f"{case}/meta"])
    model = kat_model(kat, case, step_path=path)
    state0 = {k: _np(v) for k, v in model.state_dict().items()}
    losses = _steps(model, [(kat[f"{case}/u"][k], kat[f"{case}/i"][k], kat[f"{case}/j"][k]) for k in range(ns)])
    np.testing.assert_allclose(losses, kat[f"{case}/loss"], rtol=1e-5)
    noise = NO.zero_grad_params(state0, L, bool(bn))
    skip = noise if str(kat[f"{case}/optimizer"]) == "adam" else set()
    for k, v in model.state_dict().items():
        ref = kat[f"{case}/final/p/{k}"]
        if k in skip:
            continue
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(ref), (k, int(v), int(ref))
        else:
            assert close(_np(v), ref, 1e-5), (case, k, np.abs(_np(v) - ref).max())
            du, dr = _np(v) - state0[k], ref - state0[k]         # the updates themselves, relative to their size
            if k not in noise:                                      # (an update of rounding noise has no size to compare to)
                assert np.abs(du - dr).max() <= 1e-3 * max(np.abs(dr).max(), 1e-30), (case, k, np.abs(du - dr).max())


@pytest.mark.parametrize("bn", [1, 0])
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_rank_full_rank_predict(kat, bn, mode):
    from daisyrec_amd.model import NFM
    from daisyrec_amd.utils.dataset import CandidatesDataset, get_dataloader
    U, I, f, C, nB, topk = (int(x) for x in kat["rank/meta"])
    key = f"rank/bn{bn}_{mode}"
    model = NFM(nfm_config(user_num=U, item_num=I, factors=f, num_layers=2, batch_norm=bool(bn), dropout=0.0, topk=topk))
    model.load_state_dict({k: torch.from_numpy(kat[f"{key}/before/p/{k}"].copy()) for k in model.state_dict()})
    model.train(mode == "train")
    us, cands = kat["rank/us"], kat["rank/cands"]
    loader = get_dataloader(CandidatesDataset([[int(us[b]), cands[b]] for b in range(nB)]), batch_size=4, shuffle=False,
                            num_workers=0)
    np.testing.assert_array_equal(model.rank(loader), kat[f"{key}/preds"])
    np.testing.assert_array_equal(np.stack([model.full_rank(int(u)) for u in us]), kat[f"{key}/full"])
    if not bn:
        pr = np.array([model.predict(int(us[b]), int(cands[b, 0])) for b in range(nB)], dtype=np.float32)
        np.testing.assert_allclose(pr, kat[f"{key}/predict"], rtol=1e-5, atol=1e-6)
    else:
        with pytest.raises(ValueError, match="expected 2D or 3D input"):
            model.predict(int(us[0]), int(cands[0, 0]))
    for k, v in model.state_dict().items():              # training mode: the running statistics moved as the reference's
        ref = kat[f"{key}/after/p/{k}"]
        assert close(_np(v), ref, 1e-5) if v.is_floating_point() else int(v) == int(ref), k


def test_ml100k_first_50_batches(kat):
    """test.py --algo_name nfm (nfm.yaml, no dropout): one epoch over the reference's first 12 800 triples, in the
    loader's order.  The trajectory is sensitive to rounding after ~30 steps (the float64 oracle itself is 0.15% off the
    reference's loss at batch 40): the first 25 batch losses are held to 1e-5, the epoch loss to 1%."""
    from daisyrec_amd.model import NFM
    from daisyrec_amd.utils.dataset import BasicDataset, get_dataloader
    g = kat
    U, I, f, L = (int(x) for x in g["ml/meta"])
    lr, r1, r2 = (float(x) for x in g["ml/hyper"])
    models = []
    for _ in range(2):
        torch.set_rng_state(torch.from_numpy(g["ml/rng_state_before_model"]))
        models.append(NFM(nfm_config(user_num=U, item_num=I, factors=f, num_layers=L, lr=lr, reg_1=r1, reg_2=r2,
                                     epochs=1, dropout=0.0, seed=int(g["ml/seed"]))))
    loader = get_dataloader(BasicDataset(g["ml/samples"]), batch_size=int(g["ml/batch_size"]), shuffle=True,
                            num_workers=0)
    torch.set_rng_state(torch.from_numpy(g["ml/rng_state_before_fit"]))
    models[0].fit(loader)
    ref = float(g["ml/epoch_losses"][0])
    assert abs(models[0].epoch_losses[0] - ref) <= 1e-2 * abs(ref), (models[0].epoch_losses, ref)
    torch.set_rng_state(torch.from_numpy(g["ml/rng_state_before_fit"]))
    perm = models[1]._epoch_order(loader, len(g["ml/samples"]))
    t = g["ml/samples"][perm.numpy()]
    B = int(g["ml/batch_size"])
    models[1].train()
    losses = _steps(models[1], [(t[s:s + B, 0], t[s:s + B, 1], t[s:s + B, 2]) for s in range(0, 25 * B, B)])
    np.testing.assert_allclose(losses, g["ml/batch_losses"][:25], rtol=1e-5)


def _random_model(rng, U, I, d, L, bn=True, act="relu", **over):
    from daisyrec_amd.model import NFM
    torch.manual_seed(int(rng.integers(1 << 30)))
    m = NFM(nfm_config(user_num=U, item_num=I, factors=d, num_layers=L, batch_norm=bn, act_function=act, **over))
    with torch.no_grad():
        for p in (m.u_bias.weight, m.i_bias.weight):
            p.copy_(0.1 * torch.randn_like(p))
    return m


def _oracle_check(model, u, i, j, masks=None, p=0.0, rtol=1e-4, update_rtol=None):
    """one step against float64; update_rtol: compare the parameter updates (relative to the largest update of the
    tensor) instead of the parameters"""
    state0 = {k: _np(v).copy() for k, v in model.state_dict().items()}
    noise = NO.zero_grad_params(state0, model.num_layers, model.batch_norm) if update_rtol is not None else set()
    losses = _steps(model, [(u, i, j)])
    ol, params, bufs = NO.run_steps(state0, [(u, i, j)], model.num_layers, model.batch_norm, model.act_function,
                                    model.loss_type, model._resolve_optimizer(), model.lr, model.reg_1, model.reg_2,
                                    masks=[masks] if masks is not None else None, p=p)
    assert abs(losses[0] - ol[0]) <= rtol * abs(ol[0]), (losses, ol)
    for k, v in model.state_dict().items():
        ref = {**params, **bufs}[k].numpy()
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(ref), k
        elif k in noise:              # exact gradient 0: an update of rounding noise, no two implementations agree on it
            continue
        elif update_rtol is not None:
            du, dr = _np(v) - state0[k], ref - state0[k]
            assert np.abs(du - dr).max() <= update_rtol * max(np.abs(dr).max(), 1e-30), (k, np.abs(du - dr).max())
        else:
            assert close(_np(v), ref, rtol), (k, np.abs(_np(v) - ref).max())


def test_dropout_half_against_the_oracle_with_the_device_masks():
    from daisyrec_amd import ops
    from daisyrec_amd import _native as N
    rng = np.random.default_rng(5)
    U, I, d, L, B = 60, 70, 30, 2, 256
    model = _random_model(rng, U, I, d, L, dropout=0.5, reg_1=1e-3, reg_2=1e-3)
    u, i, j = (rng.integers(0, n, B).astype(np.int32) for n in (U, I, I))
    seed = 1                                            # _steps: step k uses seed k + 1
    keep = {s: _np(ops.dropout_mask(seed, N.NFM_DROP_STREAM + s, 2 * B * d, 0.5)).reshape(2 * B, d).astype(bool)
            for s in range(L + 1)}
    rate = np.mean([k.mean() for k in keep.values()])
    n = (L + 1) * 2 * B * d
    assert abs(rate - 0.5) <= 3 * np.sqrt(0.25 / n), rate
    masks = ({s: keep[s][:B] for s in keep}, {s: keep[s][B:] for s in keep})
    _oracle_check(model, u, i, j, masks=masks, p=0.5)


@pytest.mark.parametrize("d,L,act,loss", [(7, 3, "tanh", "BPR"), (64, 2, "relu", "TL"), (30, 1, "sigmoid", "SL"),
                                          (256, 1, "relu", "BPR"), (1, 2, "elu", "HL")])
def test_shapes_against_the_oracle(d, L, act, loss):
    rng = np.random.default_rng(d * 10 + L)
    U, I, B = 50, 80, 100
    model = _random_model(rng, U, I, d, L, act=act, loss_type=loss, dropout=0.0, reg_1=1e-3, reg_2=1e-3, lr=0.05)
    u, i = (rng.integers(0, n, B).astype(np.int32) for n in (U, I))
    j = (rng.integers(0, 2, B) if loss in ("CL", "SL") else rng.integers(0, I, B)).astype(np.int32)
    _oracle_check(model, u, i, j)


def test_large_batch_step_against_the_oracle():
    """the step at B = 65 536, d = 64 (two calls of 65 536 rows each) against float64"""
    rng = np.random.default_rng(11)
    U, I, d, L, B = 6000, 3700, 64, 2, 65536
    model = _random_model(rng, U, I, d, L, dropout=0.0, lr=0.01)
    u, i, j = (rng.integers(0, n, B).astype(np.int32) for n in (U, I, I))
    # fp32 against float64: the first stage's batch std is ~0.01 (products of two embeddings), so BatchNorm's 1/std
    # (~100) scales the fp32 rounding of the products and of everything downstream - the updates are compared relative
    # to their size (measured 2.6e-3 with fp64 column sums in both directions: the sums are not what limits it)
    _oracle_check(model, u, i, j, rtol=1e-4, update_rtol=5e-3)


def _fit(seed, dropout=0.5):
    from daisyrec_amd.utils.dataset import BasicDataset, get_dataloader
    rng = np.random.default_rng(seed)
    U, I = 90, 120
    model = _random_model(rng, U, I, 30, 2, dropout=dropout, epochs=2, seed=seed)
    t = np.stack([rng.integers(0, U, 1000), rng.integers(0, I, 1000), rng.integers(0, I, 1000)], 1).astype(np.int32)
    torch.manual_seed(seed)
    model.fit(get_dataloader(BasicDataset(t), batch_size=128, shuffle=True, num_workers=0))
    return model


def test_two_seeded_fits_are_bitwise_equal():
    a, b = _fit(3), _fit(3)
    assert a.epoch_losses == b.epoch_losses
    for k, v in a.state_dict().items():
        assert np.array_equal(np.atleast_1d(_np(v)).view(np.uint8), np.atleast_1d(_np(b.state_dict()[k])).view(np.uint8)), k


def test_fit_epoch_loss_is_the_sum_of_the_step_losses():
    """fit's epoch loss (summed on the device over the steps the library issues) = the losses of the same steps taken one
    by one (step k with dropout key (seed << 32) | k), and calc_loss of the first batch = the first step's loss."""
    from daisyrec_amd.utils.dataset import BasicDataset, get_dataloader
    rng = np.random.default_rng(9)
    U, I, B, seed = 70, 90, 100, 5
    t = np.stack([rng.integers(0, U, 950), rng.integers(0, I, 950), rng.integers(0, I, 950)], 1).astype(np.int32)
    a, b, c = (_random_model(np.random.default_rng(4), U, I, 30, 2, dropout=0.5, epochs=1, seed=seed) for _ in range(3))
    a.fit(get_dataloader(BasicDataset(t), batch_size=B, shuffle=False, num_workers=0))
    batches = [(t[s:s + B, 0], t[s:s + B, 1], t[s:s + B, 2]) for s in range(0, len(t), B)]
    losses = _steps(b, batches, seed_steps=[(seed << 32) | (k + 1) for k in range(len(batches))])
    assert abs(a.epoch_losses[0] - sum(losses)) <= 1e-9 * abs(sum(losses)), (a.epoch_losses, sum(losses))
    for k, v in a.state_dict().items():
        assert np.array_equal(np.atleast_1d(_np(v)).view(np.uint8), np.atleast_1d(_np(b.state_dict()[k])).view(np.uint8)), k
    c.train()
    first = float(c.calc_loss([torch.from_numpy(x.copy()) for x in batches[0]]).cpu())
    assert first == losses[0]


@pytest.mark.parametrize("opt", ["sgd", "adam", "adagrad", "rmsprop"])
def test_fit_epoch_equals_step_grads_plus_the_dense_optimiser(opt):
    """daisy_nfm_fit_epoch against daisy_nfm_step_grads + daisy_{sgd,adam,adagrad,rmsprop}_dense issued step by step:
    the flat parameters, the optimiser state and the BatchNorm buffers bit for bit.  20 triples in batches of 7 (three
    steps, the last one partial), starting at optimiser step 5 and dropout step 9: a loop that fed Adam the dropout
    counter, or the count from 0, would show in the bias correction."""
    from daisyrec_amd import ops
    from daisyrec_amd import _native as N
    rng = np.random.default_rng(13)
    U, I, d, L, n, B, seed, t0, s0 = 11, 13, 8, 1, 20, 7, 5, 5, 9
    tri = [_i32(rng.integers(0, m, n)) for m in (U, I, I)]

    def run(native):
        model = _random_model(np.random.default_rng(4), U, I, d, L, dropout=0.0, reg_1=1e-3, reg_2=1e-3, lr=0.01)
        p = model._params()
        init = _np(model._flat).copy()
        gflat = torch.zeros_like(model._flat)
        g = model._grad_table(gflat)
        loss_id = ops.LOSS_IDS[model.loss_type.upper()]
        optim = ops.DenseOptimizer(opt, model.lr)
        optim.t = t0
        ctx = model._ctx(B)
        try:
            if native:
                steps = ctx.fit_epoch(p, g, model._bn(), *tri, B, optim, model._flat, gflat, loss_id, model.reg_1, model.reg_2,
                                      dropout=0.0, seed_hi=seed << 32, step0=s0)
            else:
                steps = 0
                for b0 in range(0, n, B):
                    steps += 1
                    ctx.step_grads(p, g, model._bn(), *(t[b0:b0 + B] for t in tri), loss_id, model.reg_1, model.reg_2,
                                   dropout=0.0, seed=(seed << 32) | (s0 + steps))
                    optim.next_step()
                    optim.step(model._flat, gflat)
            loss = float(ctx.stats[N.NFST_LOSS_SUM].cpu())
        finally:
            ctx.close()
        bufs = [_np(x).copy() for row in model._bn() for x in row]
        return steps, optim.t, loss, _np(model._flat).copy(), [_np(x).copy() for x in optim.state_for(model._flat)], bufs, init

    a, b = run(True), run(False)
    assert a[0] == b[0] == 3 and a[1] == b[1] == t0 + 3
    assert a[2] == b[2] and np.isfinite(a[2]) and a[2] > 0
    assert np.array_equal(a[3].view(np.uint8), b[3].view(np.uint8)) and not np.array_equal(a[3], a[6])
    assert len(a[4]) == len(b[4]) == {"sgd": 0, "adam": 2, "adagrad": 1, "rmsprop": 1}[opt]
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a[4], b[4]))
    assert len(a[5]) == 3 * (L + 1) and all(np.array_equal(x, y) for x, y in zip(a[5], b[5]))


def test_one_row_batch_with_batch_norm_raises():
    from daisyrec_amd.utils.dataset import BasicDataset, get_dataloader
    rng = np.random.default_rng(2)
    m = _random_model(rng, 20, 30, 8, 1, dropout=0.0, epochs=1)
    t = np.stack([rng.integers(0, 20, 9), rng.integers(0, 30, 9), rng.integers(0, 30, 9)], 1).astype(np.int32)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        m.fit(get_dataloader(BasicDataset(t), batch_size=4, shuffle=False, num_workers=0))


def _one_step_state(path, rng_seed=21):
    rng = np.random.default_rng(rng_seed)
    U, I, B = 40, 60, 200
    model = _random_model(rng, U, I, 30, 2, dropout=0.5, reg_1=1e-3, reg_2=1e-3, step_path=path, optimizer="adam", lr=0.01)
    u, i, j = (rng.integers(0, n, B).astype(np.int32) for n in (U, I, I))
    losses = _steps(model, [(u, i, j), (u[::-1].copy(), j, i)])
    return losses, {k: _np(v).copy() for k, v in model.state_dict().items()}


def test_small_and_layered_paths_give_the_same_bits():
    (la, sa), (lb, sb) = _one_step_state("small"), _one_step_state("layered")
    assert la == lb
    for k in sa:
        assert np.array_equal(np.atleast_1d(sa[k]).view(np.uint8), np.atleast_1d(sb[k]).view(np.uint8)), k


def test_forced_small_path_refuses_a_large_batch():
    from daisyrec_amd import _native as N
    rng = np.random.default_rng(1)
    model = _random_model(rng, 20, 30, 8, 1, dropout=0.0, step_path="small")
    u, i, j = (rng.integers(0, 20, 300).astype(np.int32) for _ in range(3))
    with pytest.raises(Exception, match="small path"):
        _steps(model, [(u, i, j)])
    assert N.NFM_SMALL_MAX_B == 256


@pytest.mark.parametrize("opt", ["adagrad", "rmsprop"])
def test_adagrad_rmsprop_against_the_oracle(opt):
    rng = np.random.default_rng(31)
    U, I, B = 50, 70, 128
    model = _random_model(rng, U, I, 16, 2, bn=False, act="tanh", dropout=0.0, optimizer=opt, lr=1e-3)
    u, i, j = (rng.integers(0, n, B).astype(np.int32) for n in (U, I, I))
    _oracle_check(model, u, i, j, rtol=1e-4, update_rtol=1e-3)


def test_second_fit_restarts_adam():
    """the reference's fit builds a fresh torch.optim.Adam: bias correction starts over at t = 1 in every fit"""
    from daisyrec_amd.utils.dataset import BasicDataset, get_dataloader
    rng = np.random.default_rng(13)
    U, I = 30, 40
    t = np.stack([rng.integers(0, U, 400), rng.integers(0, I, 400), rng.integers(0, I, 400)], 1).astype(np.int32)
    a, b = (_random_model(np.random.default_rng(6), U, I, 16, 1, dropout=0.0, optimizer="adam", lr=0.01, epochs=1)
            for _ in range(2))
    loader = get_dataloader(BasicDataset(t), batch_size=100, shuffle=False, num_workers=0)
    a.fit(loader)
    a.fit(loader)
    b.fit(loader)
    b.train()
    _steps(b, [(t[s:s + 100, 0], t[s:s + 100, 1], t[s:s + 100, 2]) for s in range(0, 400, 100)])   # a fresh Adam
    for k, v in a.state_dict().items():
        assert np.array_equal(np.atleast_1d(_np(v)).view(np.uint8), np.atleast_1d(_np(b.state_dict()[k])).view(np.uint8)), k


@pytest.mark.parametrize("bn", [True, False])
def test_torch_op_nfm_scores_equals_the_mirror(bn):
    import daisyrec_amd.torch_ops  # noqa: F401
    from daisyrec_amd import _native as N
    rng = np.random.default_rng(17)
    U, I = 30, 500
    m = _random_model(rng, U, I, 24, 2, bn=bn, act="sigmoid", dropout=0.0)
    m.eval()
    p = m._params()
    users = torch.tensor([3], device=DEV)
    ref = m._scores(users, None, C_=0, n=I)
    L = m.num_layers
    bns = m._bn() or []
    out = torch.ops.daisyrec.nfm_scores(p["P"], p["Q"], p["ub"], p["ib"], p["bias"], p["wp"],
                                        [p[f"W{l}"] for l in range(1, L + 1)], [p[f"b{l}"] for l in range(1, L + 1)],
                                        [p[f"bn_w{s}"] for s in range(L + 1)] if bn else [],
                                        [p[f"bn_b{s}"] for s in range(L + 1)] if bn else [],
                                        [x[0] for x in bns], [x[1] for x in bns], users, None, 0, I, N.NFM_ACT["sigmoid"])
    assert torch.equal(out, ref)
    us = torch.arange(4, device=DEV)
    cands = torch.randint(0, I, (4 * 7,), device=DEV)
    ref2 = m._scores(us, cands, C_=7)
    out2 = torch.ops.daisyrec.nfm_scores(p["P"], p["Q"], p["ub"], p["ib"], p["bias"], p["wp"],
                                         [p[f"W{l}"] for l in range(1, L + 1)], [p[f"b{l}"] for l in range(1, L + 1)],
                                         [p[f"bn_w{s}"] for s in range(L + 1)] if bn else [],
                                         [p[f"bn_b{s}"] for s in range(L + 1)] if bn else [],
                                         [x[0] for x in bns], [x[1] for x in bns], us, cands, 7, 0, N.NFM_ACT["sigmoid"])
    assert torch.equal(out2, ref2)
