"""NeuMF widening on the GPU: the HIP path through the C ABI against the golden
vectors of the REAL reference NeuMF (tests/golden/kat_neumf.npz) and the CPU oracle.
Tolerances: loss within 1e-5 relative per step; parameters at fp32 round-off (SGD) or, under Adam,
round-off for all but the few elements whose gradient is ~0 (see tests/test_oracle_neumf.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import bpr_mf_numpy as O
from oracle import neumf_numpy as NO
from test_oracle_neumf import assert_params_close, load_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def kat_neumf():
    return np.load(os.path.join(HERE, "golden", "kat_neumf.npz"))


def _dev(p):
    return {k: torch.as_tensor(np.ascontiguousarray(v)).to(DEV) for k, v in p.items()}


@pytest.mark.parametrize("M,N,K", [(128, 128, 16), (1, 1, 1), (257, 96, 48), (1000, 24, 48), (333, 256, 512),
                                   (4096, 64, 128), (70, 130, 9)])
def test_mfma_gemm_nt(M, N, K):
    """The fp32 MFMA tile kernel of the MLP tower against torch (fp64 reference)."""
    from daisyrec_amd import ops
    g = torch.Generator(device=DEV)
    g.manual_seed(M * 7 + N)
    A = torch.randn(M, K, device=DEV, generator=g)
    B = torch.randn(N, K, device=DEV, generator=g)
    got = ops.gemm_nt(A, B)
    want = (A.double() @ B.double().T)
    assert float((got.double() - want).abs().max()) <= 2e-6 * K * float(want.abs().max() + 1)


def _run_case(g, name, ops, dropout=0.0):
    U, I, d, L, B, ns = (int(x) for x in g[f"{name}/meta"])
    lr, r1, r2 = (float(x) for x in g[f"{name}/hyper"])
    lt = ops.loss_id(str(g[f"{name}/loss_type"]))
    model = str(g[f"{name}/model"])
    names = ops.neumf_param_names(L)
    p = _dev(load_params(g, name, L, "0"))
    grads = {k: torch.zeros_like(v) for k, v in p.items()}
    is_adam = str(g[f"{name}/optimizer"]) == "adam"
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v = {k: torch.zeros_like(v) for k, v in p.items()}
    ctx = ops.NeumfContext(2 * B, d, L, U, I, model=model)
    losses = []
    for s in range(ns):
        u, i, j = (torch.as_tensor(g[f"{name}/{k}"][s]).to(DEV) for k in "uij")
        ctx.step_grads(p, grads, u, i, j, lt, r1, r2, dropout=dropout, seed=1000 + s)
        losses.append(float(ctx.stats[11].cpu()))
        for k in names:
            if is_adam:
                ops.adam_dense(p[k], grads[k], m[k], v[k], lr, s + 1)
            else:
                ops.sgd_dense(p[k], grads[k], lr)
    ctx.close()
    return {k: t.cpu().numpy() for k, t in p.items()}, losses, is_adam, lr, ns, names


def test_neumf_kat_steps(kat_neumf):
    from daisyrec_amd import ops
    g = kat_neumf
    for name in g["names"]:
        name = str(name)
        p, losses, is_adam, lr, ns, names = _run_case(g, name, ops)
        for s, loss in enumerate(losses):
            ref = float(g[f"{name}/loss"][s])
            assert abs(loss - ref) <= 1e-5 * abs(ref), (name, s, loss, ref)
        # Adam: gradients that cancel pairwise under BPR (a bias of a unit that is active on both rows of
        # every sample) are pure rounding residue in BOTH implementations and Adam turns their sign into
        # a +-lr step, so up to ~10 % of a small bias vector may legitimately differ by <= 2*lr*steps
        assert_params_close(p, {k: g[f"{name}/{k}"] for k in names}, names, name, 5e-6,
                            adam_lr=lr if is_adam else None, steps=ns, frac=0.9)


def test_neumf_rank_kat(kat_neumf):
    from daisyrec_amd import ops
    g = kat_neumf
    U, I, d, L = (int(x) for x in g["rank/meta"])
    p_np = load_params(g, "rank", L)
    p = _dev(p_np)
    us, cands, topk = g["rank/us"], g["rank/cands"], int(g["rank/topk"])
    B, C = cands.shape
    ctx = ops.NeumfContext(300, d, L, U, I)          # smaller than B*C: exercises the chunked scoring
    scores = ctx.scores(p, torch.as_tensor(us).to(DEV), torch.as_tensor(cands).reshape(-1).to(DEV), C_=C)
    _, want = NO.neumf_rank(p_np, us, cands, topk, L)
    np.testing.assert_allclose(scores.cpu().numpy().reshape(B, C), want, rtol=1e-5, atol=2e-6)
    out = ops.topk_from_scores(scores.view(B, C), torch.as_tensor(cands).to(DEV), topk).cpu().numpy()
    assert (out.astype(np.float32) == g["rank/preds"]).mean() > 0.99
    full_scores = ctx.scores(p, torch.as_tensor(us[:1]).to(DEV), None, C_=0, n=I)
    full = ops.full_topk_from_scores(full_scores, topk).cpu().numpy()
    assert (full == g["rank/full"][0]).mean() >= 0.9
    pp = ctx.scores(p, torch.as_tensor(us).to(DEV), torch.as_tensor(cands[:, 0].copy()).to(DEV))
    np.testing.assert_allclose(pp.cpu().numpy(), g["rank/predict"], rtol=1e-5, atol=2e-6)
    ctx.close()


@pytest.mark.parametrize("model,loss", [("NeuMF", "BPR"), ("MLP", "CL")])
def test_neumf_dropout_step_matches_oracle_with_the_same_masks(model, loss):
    """Training mode: the device's dropout masks (counter hash) restated by the oracle."""
    from daisyrec_amd import ops
    rng = np.random.default_rng(3)
    U, I, d, L, B, pdrop, seed = 40, 30, 8, 3, 50, 0.5, 77
    dm = d << (L - 1)
    shapes = {"uG": (U, d), "iG": (I, d), "uM": (U, dm), "iM": (I, dm), "Wp": (1, d if model == "MLP" else 2 * d),
              "bp": (1,)}
    w = 2 * dm
    for l in range(1, L + 1):
        shapes[f"W{l}"], shapes[f"b{l}"] = (w // 2, w), (w // 2,)
        w //= 2
    p_np = {k: (rng.standard_normal(s) * 0.3).astype(np.float32) for k, s in shapes.items()}
    u, i = rng.integers(0, U, B).astype(np.int32), rng.integers(0, I, B).astype(np.int32)
    lt = O.LOSS_IDS[loss]
    j = (rng.integers(0, 2, B) if loss == "CL" else rng.integers(0, I, B)).astype(np.int32)
    mp = NO.dropout_masks(seed, np.arange(B), d, L, pdrop)
    mn = NO.dropout_masks(seed, np.arange(B, 2 * B), d, L, pdrop)
    assert 0.4 < np.mean(mp[0] > 0) < 0.6
    want_loss, want = NO.neumf_grad(p_np, u, i, j, 1e-3, 1e-3, L, lt, model, masks_pos=mp, masks_neg=mn)
    p = _dev(p_np)
    grads = {k: torch.zeros_like(v) for k, v in p.items()}
    ctx = ops.NeumfContext(2 * B, d, L, U, I, model=model)
    ctx.step_grads(p, grads, *(torch.as_tensor(x).to(DEV) for x in (u, i, j)), lt, 1e-3, 1e-3, dropout=pdrop, seed=seed)
    assert abs(float(ctx.stats[11].cpu()) - want_loss) <= 1e-5 * abs(want_loss)
    for k in shapes:
        np.testing.assert_allclose(grads[k].cpu().numpy(), want[k], rtol=2e-4, atol=2e-5, err_msg=k)
    ctx.close()


def _neumf_cfg(g, prefix, **over):
    from conftest import mf_config
    U, I, d, L = (int(x) for x in g[f"{prefix}/meta"])
    lr, r1, r2 = (float(x) for x in g[f"{prefix}/hyper"])
    cfg = mf_config(user_num=U, item_num=I, factors=d, num_layers=L, lr=lr, reg_1=r1, reg_2=r2, dropout=0.0,
                    model_name="NeuMF", GMF_model=None, MLP_model=None, algo_name="neumf",
                    epochs=int(g[f"{prefix}/epochs"]), optimizer=str(g[f"{prefix}/optimizer"]))
    cfg.update(over)
    return cfg, L


def _fit_like_the_reference(g, prefix):
    from daisyrec_amd.model.NeuMFRecommender import NeuMF
    from daisyrec_amd.utils.dataset import BasicDataset, CandidatesDataset, get_dataloader
    cfg, L = _neumf_cfg(g, prefix)
    torch.manual_seed(int(g[f"{prefix}/seed"]))
    model = NeuMF(cfg)
    for k, p in model._named().items():               # same module order + RNG stream => same init
        np.testing.assert_array_equal(p.detach().numpy(), g[f"{prefix}/{k}0"], err_msg=k)
    loader = get_dataloader(BasicDataset(g["ml/samples"]), batch_size=int(g[f"{prefix}/batch_size"]), shuffle=True,
                            num_workers=4)
    torch.set_rng_state(torch.from_numpy(g[f"{prefix}/rng_state_before_fit"]))
    model.fit(loader)
    ucands = [[int(u), c] for u, c in zip(g["ml/test_u"], g["ml/cands"])]
    preds = model.rank(get_dataloader(CandidatesDataset(ucands), batch_size=128, shuffle=False, num_workers=0))
    return model, preds, L


def test_neumf_ml100k_sgd_through_the_dropin(kat_neumf):
    """run_examples/test.py --algo_name neumf --optimizer sgd (dropout 0) on ml-100k (first 100 batches: see
    tests/golden/make_golden_neumf.py) through NeuMF.fit / NeuMF.rank with the reference's triples, init
    and DataLoader order: epoch loss within 1e-5, parameters at round-off, ranked top-N identical."""
    g = kat_neumf
    model, preds, L = _fit_like_the_reference(g, "mlsgd")
    ref = float(g["mlsgd/epoch_losses"][0])
    assert abs(model.epoch_losses[0] - ref) <= 1e-5 * abs(ref), (model.epoch_losses, ref)
    for k, p in model._named().items():
        np.testing.assert_allclose(p.detach().cpu().numpy(), g[f"mlsgd/{k}1"], atol=3e-5, err_msg=k)
    assert preds.dtype == np.float32 and preds.shape == g["mlsgd/preds"].shape
    same = (preds == g["mlsgd/preds"]).all(axis=1).mean()
    assert same > 0.98, f"top-N lists identical for {same:.3f} of the users"
    # predict / full_rank / calc_loss agree with the oracle on the trained parameters
    p_np = {k: p.detach().cpu().numpy() for k, p in model._named().items()}
    want, _ = NO.neumf_forward(p_np, [3], [5], L)
    assert abs(model.predict(3, 5) - float(want[0])) < 1e-5
    full = model.full_rank(int(g["ml/test_u"][0]))
    assert (full == NO.neumf_full_rank(p_np, int(g["ml/test_u"][0]), model.topk, L)).mean() > 0.9
    b = g["ml/samples"][:256]
    model.eval()
    loss = float(model.calc_loss([torch.from_numpy(b[:, k].copy()) for k in range(3)]).cpu())
    want_loss, _ = NO.neumf_grad(p_np, b[:, 0], b[:, 1], b[:, 2], model.reg_1, model.reg_2, L)
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss)


def test_neumf_ml100k_adam_defaults(kat_neumf):
    """neumf.yaml defaults (Adam lr 0.001; dropout 0), 100 batches: epoch loss within 1e-5, ranked lists
    identical for >= 90 % of the users (Adam's sign-like first steps amplify round-off in a few rows)."""
    g = kat_neumf
    model, preds, L = _fit_like_the_reference(g, "ml")
    ref = float(g["ml/epoch_losses"][0])
    assert abs(model.epoch_losses[0] - ref) <= 1e-5 * abs(ref), (model.epoch_losses, ref)
    same = (preds == g["ml/preds"]).all(axis=1).mean()
    assert same > 0.9, f"top-N lists identical for {same:.3f} of the users"


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_neumf_ml100k_d64_fit_against_the_reference(precision):
    """ml-100k at the BASELINE configs[3] tower shape (factors 64, 3 layers, batches of 2048 samples = 4096 rows > the 2095
    table rows: the first layer runs through the tables, and in bf16 the fused tower kernel takes the step) against the
    REFERENCE's own fit (tests/golden/kat_neumf_d64.npz, make_golden_neumf_d64.py): same triples, init, DataLoader order.
    fp32: epoch loss within 1e-5, the step of every parameter at round-off, ranked lists identical.  bf16 (round 6, the mode
    configs[3] names): the epoch loss within 5e-5 of the reference's, every parameter's 12-step change within 6 % of the
    reference's (bf16's own distance: 2.3 ... 3.7 %) and within 2.5 % of the ORACLE's replay of the fit with the same bf16 roundings
    (that replay's loss to 1e-5); the ranked lists keep their members, not their order (see below)."""
    from daisyrec_amd.model.NeuMFRecommender import NeuMF
    from daisyrec_amd.utils.dataset import BasicDataset, CandidatesDataset, get_dataloader
    from conftest import mf_config
    g = np.load(os.path.join(HERE, "golden", "kat_neumf_d64.npz"))
    U, I, d, L = (int(x) for x in g["meta"])
    lr, r1, r2 = (float(x) for x in g["hyper"])
    cfg = mf_config(user_num=U, item_num=I, factors=d, num_layers=L, lr=lr, reg_1=r1, reg_2=r2, dropout=0.0, model_name="NeuMF",
                    GMF_model=None, MLP_model=None, algo_name="neumf", epochs=1, optimizer=str(g["optimizer"]),
                    precision=precision)
    torch.manual_seed(int(g["seed"]))
    model = NeuMF(cfg)
    init = {k: p.detach().cpu().numpy().copy() for k, p in model._named().items()}
    for k, p0 in init.items():                        # same module order + RNG stream => same init (checksums of the reference's)
        np.testing.assert_allclose([p0.astype(np.float64).sum(), np.abs(p0.astype(np.float64)).sum()], g[f"{k}0_sum"], rtol=1e-12)
    loader = get_dataloader(BasicDataset(g["samples"]), batch_size=int(g["batch_size"]), shuffle=True, num_workers=4)
    torch.set_rng_state(torch.from_numpy(g["rng_state_before_fit"]))
    model.fit(loader)
    ref = float(g["epoch_losses"][0])
    assert abs(model.epoch_losses[0] - ref) <= (1e-5 if precision == "fp32" else 5e-5) * abs(ref), (precision, model.epoch_losses, ref)

    def step_error(want_delta):
        worst = {}
        for k, p in model._named().items():
            rows = g[f"{k}_delta"].shape[0]
            delta = (p.detach().cpu().numpy() - init[k])[:rows]
            worst[k] = float(np.linalg.norm(delta - want_delta[k][:rows]) / max(np.linalg.norm(want_delta[k][:rows]), 1e-30))
        return worst

    vs_ref = step_error({k: g[f"{k}_delta"] for k in init})
    if precision == "fp32":
        assert max(vs_ref.values()) <= 2e-3, vs_ref
        for k, p in model._named().items():
            full = float(np.linalg.norm((p.detach().cpu().numpy() - init[k]).astype(np.float64)))
            assert abs(full - float(g[f"{k}_delta_norm"])) <= 2e-3 * float(g[f"{k}_delta_norm"]), (k, full)
    else:
        # bf16 arithmetic itself sits 2.3 ... 3.7 % from the reference on the MLP parameters' 12-step change (the oracle's replay
        # with the bf16 roundings: tests/test_oracle_neumf.py states and explains it); the HIP fit follows THAT replay closely
        assert max(vs_ref.values()) <= 0.06 and vs_ref["uG"] <= 1e-3 and vs_ref["iG"] <= 1e-3, vs_ref
        from test_oracle_neumf import _replay_d64
        _, p16, init16, tot16 = _replay_d64("fact")
        assert abs(model.epoch_losses[0] - tot16) <= 1e-5 * abs(tot16), (model.epoch_losses, tot16)
        vs_replay = step_error({k: p16[k] - init16[k] for k in init})
        assert max(vs_replay.values()) <= 2.5e-2, vs_replay               # (measured 1.1 ... 1.8 %: twelve steps of the per-step 2 % pin)
    n = len(g["test_u"])
    ucands = [[int(u), c] for u, c in zip(g["test_u"], g["cands"])]
    preds = model.rank(get_dataloader(CandidatesDataset(ucands), batch_size=128, shuffle=False, num_workers=0))
    same = (preds[:n] == g["preds"]).all(axis=1).mean()
    if precision == "fp32":
        assert same >= 0.98, float(same)
    else:
        # twelve steps at lr 2e-5 leave the scores of a user's 1000 candidates within a few 1e-4 of each other: the ORDER of the
        # top 50 does not survive scoring with bf16-stored activations (identical lists: none), their membership largely does
        overlap = np.mean([len(set(a.tolist()) & set(b.tolist())) / a.shape[0] for a, b in zip(preds[:n], g["preds"])])
        assert overlap >= 0.5, (float(same), float(overlap))
        print(f"bf16 top-{preds.shape[1]} overlap with the reference: {overlap:.3f}, identical lists: {same:.3f}")


def test_neumf_dropout_training_runs_and_learns(kat_neumf):
    """neumf.yaml's dropout 0.5 with the device masks: the loss goes down, eval-mode scoring is deterministic."""
    from daisyrec_amd.model.NeuMFRecommender import NeuMF
    from daisyrec_amd.utils.dataset import BasicDataset, get_dataloader
    g = kat_neumf
    cfg, L = _neumf_cfg(g, "ml", dropout=0.5, epochs=2)
    torch.manual_seed(0)
    model = NeuMF(cfg)
    loader = get_dataloader(BasicDataset(g["ml/samples"]), batch_size=1024, shuffle=True, num_workers=0)
    model.fit(loader)
    assert model.epoch_losses[1] < model.epoch_losses[0]
    a = model.forward(torch.arange(50), torch.arange(50)).cpu()
    b = model.forward(torch.arange(50), torch.arange(50)).cpu()
    assert torch.equal(a, b)
    for name in ("GMF", "MLP"):
        m2 = NeuMF({**cfg, "model_name": name, "epochs": 1, "dropout": 0.0})
        m2.fit(loader)
        assert np.isfinite(m2.epoch_losses[0])


@pytest.mark.parametrize("M,N,K", [(256, 128, 64), (1024, 256, 512), (384, 64, 96), (128, 128, 32), (512, 64, 128)])
def test_mfma_gemm_nt_bf16_mode(M, N, K):
    """bf16-input MFMA variant: exact product of the bf16-rounded operands (fp32 accumulation), asymmetric B.
    (N a multiple of 64: narrower products - a tower's last layers at factors < 64 - take the exact fp32 kernel instead,
    measured in round 6: |result - fp64 product| <= 2e-5 at N = 8 ... 96.)"""
    from daisyrec_amd import ops
    g = torch.Generator(device=DEV)
    g.manual_seed(M + K)
    A = torch.randn(M, K, device=DEV, generator=g)
    B = torch.randn(N, K, device=DEV, generator=g) + torch.arange(N, device=DEV).view(-1, 1) * 0.01
    got = ops.gemm_nt(A, B, bf16=True)
    want = A.bfloat16().double() @ B.bfloat16().double().T
    assert float((got.double() - want).abs().max()) <= 1e-5 * K * float(want.abs().max() + 1)
    exact = A.double() @ B.double().T
    assert float((got.double() - exact).abs().max()) <= 2e-2 * float(exact.abs().max())      # bf16 rounding only


def _tower_shapes(U, I, d, L):
    dm = d << (L - 1)
    shapes = {"uG": (U, d), "iG": (I, d), "uM": (U, dm), "iM": (I, dm), "Wp": (1, 2 * d), "bp": (1,)}
    w = 2 * dm
    for l in range(1, L + 1):
        shapes[f"W{l}"], shapes[f"b{l}"] = (w // 2, w), (w // 2,)
        w //= 2
    return shapes


def _run_step(ops, p_np, idx, R, d, L, U, I, level, loss, env, monkeypatch, reg=1e-3):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = _dev(p_np)
    grads = {k: torch.zeros_like(v) for k, v in p.items()}
    ctx = ops.NeumfContext(R, d, L, U, I)
    ctx.set_precision(level)
    ctx.step_grads(p, grads, *idx, loss, reg, reg)
    out = float(ctx.stats[11].cpu()), {k: v.cpu().numpy() for k, v in grads.items()}
    ctx.close()
    return out


# the paths of the bf16 modes -> (precision level, environment, rounding points of oracle.neumf_numpy.neumf_grad_bf16)
BF16_PATHS = {"tower": (2, {"DAISY_NMF_FACT": "1", "DAISY_NMF_TOWER": "1"}, "fact"),
              "fact": (2, {"DAISY_NMF_FACT": "1", "DAISY_NMF_TOWER": "0"}, "fact"),
              "plain": (2, {"DAISY_NMF_FACT": "0", "DAISY_NMF_TOWER": "0"}, "plain"),
              "inputs": (1, {"DAISY_NMF_FACT": "0", "DAISY_NMF_TOWER": "0"}, "inputs")}


@pytest.mark.parametrize("path", ["tower", "fact", "plain", "inputs"])
@pytest.mark.parametrize("loss,B,scale", [(0, 256, 0.05), (0, 1024, 0.2), (3, 512, 0.1), (2, 128, 0.1), (0, 8192, 0.1)])
def test_neumf_bf16_step_against_the_bf16_oracle(path, loss, B, scale, monkeypatch):
    """Round 6: the bf16 modes pinned to an oracle that rounds to bf16 at the same points (oracle/neumf_numpy.py:
    neumf_grad_bf16 - the table products, every stored activation and back-propagated gradient, the MFMA inputs), instead of
    'within 25 % of the fp32 mode'.  What is left between the two is fp32-vs-fp64 accumulation and the rare element whose
    bf16 rounding (or ReLU gate) sits on a tie: the loss to 1e-4, every gradient to 2 % of its norm - a dropped bias term, a
    wrong scale on one layer or a missing rounding point is ten times that.  Paths: the fused tower kernel (csrc/neumf_tower.hip),
    the layer-by-layer kernels behind the table products, the plain bf16-storage step, and precision level 1.  B = 8192: 16 384
    rows = 8 split-K slices of the weight gradients - the count at which the bf16-storage GEMM remaps workgroups to tiles (until
    round 6 its slices then landed in the wrong workspace slots: partial products lost, inside the old 25 % tolerance)."""
    from daisyrec_amd import ops
    level, env, mode = BF16_PATHS[path]
    rng = np.random.default_rng(5 + B)
    U, I, d, L = 100, 80, 64, 3
    shapes = _tower_shapes(U, I, d, L)
    p_np = {k: (rng.standard_normal(s) * scale).astype(np.float32) for k, s in shapes.items()}
    u, i = (rng.integers(0, n, B).astype(np.int32) for n in (U, I))
    j = (rng.integers(0, I, B) if loss < 3 else rng.integers(0, 2, B)).astype(np.int32)
    R = B if loss >= 3 else 2 * B
    assert U + I <= R and R % 128 == 0
    want_loss, want = NO.neumf_grad(p_np, u, i, j, 1e-3, 1e-3, L, loss, bf16_points=mode)
    ref_loss, ref = NO.neumf_grad(p_np, u, i, j, 1e-3, 1e-3, L, loss)
    idx = [torch.as_tensor(x).to(DEV) for x in (u, i, j)]
    got_loss, got = _run_step(ops, p_np, idx, R, d, L, U, I, level, loss, env, monkeypatch)
    assert abs(got_loss - want_loss) <= 1e-4 * abs(want_loss), (path, got_loss, want_loss)
    worst = {}
    for k in shapes:
        nw = np.linalg.norm(want[k])
        if nw < 1e-9 * R:                           # (bp under a pairwise loss: exactly zero, here and in the oracle)
            assert np.abs(got[k]).max() <= 1e-6 * R, (path, k)
            continue
        worst[k] = (float(np.linalg.norm(got[k] - want[k]) / nw), float(np.linalg.norm(ref[k] - want[k]) / nw))
    assert all(e <= 0.02 for e, _ in worst.values()), (path, worst)
    # and the rounding really is what separates this mode from the fp64 arithmetic: the oracle's own two modes differ by more
    assert any(r > 4 * max(e, 1e-4) for e, r in worst.values()), (path, worst)


def test_neumf_tower_equals_the_layer_by_layer_step(monkeypatch):
    """the fused tower kernel against the layer-by-layer kernels it replaces (same rounding points, other summation orders):
    every gradient within 5e-3 of its norm, the loss to 1e-5, two runs of the fused step bit for bit the same, and a step of
    several tiles per workgroup (R = 64 x 700 rows > 256 workgroups) with hot table rows"""
    from daisyrec_amd import ops
    rng = np.random.default_rng(77)
    U, I, d, L = 300, 200, 64, 3
    shapes = _tower_shapes(U, I, d, L)
    p_np = {k: (rng.standard_normal(s) * 0.1).astype(np.float32) for k, s in shapes.items()}
    for B in (64, 22400):
        u, i, j = (rng.integers(0, n, B).astype(np.int32) for n in (U, I, I))
        idx = [torch.as_tensor(x).to(DEV) for x in (u, i, j)]
        if 2 * B < U + I:                            # (the table products need U + I <= R: a smaller catalogue for the small step)
            continue
        lt, gt = _run_step(ops, p_np, idx, 2 * B, d, L, U, I, 2, 0, BF16_PATHS["tower"][1], monkeypatch)
        lt2, gt2 = _run_step(ops, p_np, idx, 2 * B, d, L, U, I, 2, 0, BF16_PATHS["tower"][1], monkeypatch)
        ll, gl = _run_step(ops, p_np, idx, 2 * B, d, L, U, I, 2, 0, BF16_PATHS["fact"][1], monkeypatch)
        assert lt == lt2 and all(np.array_equal(gt[k], gt2[k]) for k in shapes)
        assert abs(lt - ll) <= 1e-5 * abs(ll), (B, lt, ll)
        for k in shapes:
            nl = np.linalg.norm(gl[k])
            if nl > 0:
                assert np.linalg.norm(gt[k] - gl[k]) <= 5e-3 * nl, (B, k, float(np.linalg.norm(gt[k] - gl[k]) / nl))


@pytest.mark.parametrize("loss,B,L,d", [(0, 256, 3, 64), (3, 300, 2, 8), (1, 128, 1, 16)])
def test_neumf_fp32_first_layer_through_the_tables(loss, B, L, d, monkeypatch):
    """Round 6: the fp32 (parity) mode also runs its first layer through the tables when the step has more rows than the
    tables (x1 = relu((T_u[user] + T_i[item]) + b1), fp32 throughout: the reference's 2 dm-term dot product associated as two
    dm-term products): against the plain fp32 step (DAISY_NMF_FACT=0) at fp32 round-off, against the fp64 oracle at the parity
    tolerance, bit for bit repeatable; widths that are no multiple of 64 and a one-layer tower included."""
    from daisyrec_amd import ops
    rng = np.random.default_rng(31 + B)
    U, I = 60, 50
    shapes = _tower_shapes(U, I, d, L)
    p_np = {k: (rng.standard_normal(s) * 0.2).astype(np.float32) for k, s in shapes.items()}
    u, i = (rng.integers(0, n, B).astype(np.int32) for n in (U, I))
    j = (rng.integers(0, I, B) if loss < 3 else rng.integers(0, 2, B)).astype(np.int32)
    R = B if loss >= 3 else 2 * B
    assert U + I <= R
    idx = [torch.as_tensor(x).to(DEV) for x in (u, i, j)]
    want_loss, want = NO.neumf_grad(p_np, u, i, j, 1e-3, 1e-3, L, loss)
    # (DAISY_NMF_MID=0: steps this small otherwise take the one-launch path of csrc/neumf_mid.hip, which has no use for the products)
    lf, gf = _run_step(ops, p_np, idx, R, d, L, U, I, 0, loss, {"DAISY_NMF_FACT": "1", "DAISY_NMF_MID": "0"}, monkeypatch)
    lf2, gf2 = _run_step(ops, p_np, idx, R, d, L, U, I, 0, loss, {"DAISY_NMF_FACT": "1", "DAISY_NMF_MID": "0"}, monkeypatch)
    lp, gp = _run_step(ops, p_np, idx, R, d, L, U, I, 0, loss, {"DAISY_NMF_FACT": "0", "DAISY_NMF_MID": "0"}, monkeypatch)
    assert lf == lf2 and all(np.array_equal(gf[k], gf2[k]) for k in shapes)
    assert abs(lf - want_loss) <= 1e-5 * abs(want_loss) and abs(lp - want_loss) <= 1e-5 * abs(want_loss)
    assert any(not np.array_equal(gf[k], gp[k]) for k in shapes)                     # the factored path really ran
    for k in shapes:
        top = np.abs(want[k]).max()
        tol = 3e-4 * top + 3e-6 * (1 + np.sqrt(R))
        assert np.abs(gf[k] - want[k]).max() <= tol, (k, float(np.abs(gf[k] - want[k]).max()), tol)
        assert np.abs(gf[k] - gp[k]).max() <= tol, (k, float(np.abs(gf[k] - gp[k]).max()), tol)


@pytest.mark.parametrize("loss,B,level,U,I", [(0, 2048, 2, 300, 200), (3, 5000, 0, 950, 1200), (0, 4096, 0, 61, 9000), (2, 2112, 2, 40, 30)])
def test_neumf_rows_grouped_by_a_counting_pass_equal_the_radix_sorts(loss, B, level, U, I, monkeypatch):
    """Round 6: the step's rows are grouped by user and by item with one stable counting pass per side (csrc/neumf_scatter.hip:
    k_cs_count / k_cs_prefix / k_cs_base / k_cs_scatter) instead of two radix sorts.  Stable = rows of one table row stay in
    ascending order = the very permutation the sorts produce, so every gradient must come out BIT FOR BIT the same with
    DAISY_NMF_COUNTING=0 (the sorts): pairwise and point-wise steps, both precisions, hot rows (40 users in 4 224 rows),
    tables near the LDS limit, a row count that is no multiple of the wave ranges."""
    from daisyrec_amd import ops
    rng = np.random.default_rng(B + U)
    d, L = 64, 3
    shapes = _tower_shapes(U, I, d, L)
    p_np = {k: (rng.standard_normal(s) * 0.1).astype(np.float32) for k, s in shapes.items()}
    u, i = (rng.integers(0, n, B).astype(np.int32) for n in (U, I))
    j = (rng.integers(0, I, B) if loss < 3 else rng.integers(0, 2, B)).astype(np.int32)
    R = B if loss >= 3 else 2 * B
    idx = [torch.as_tensor(x).to(DEV) for x in (u, i, j)]
    la, ga = _run_step(ops, p_np, idx, R, d, L, U, I, level, loss, {"DAISY_NMF_COUNTING": "1"}, monkeypatch)
    lb, gb = _run_step(ops, p_np, idx, R, d, L, U, I, level, loss, {"DAISY_NMF_COUNTING": "0"}, monkeypatch)
    assert la == lb
    for k in shapes:
        assert np.array_equal(ga[k], gb[k]), k
    want_loss, want = NO.neumf_grad(p_np, u, i, j, 1e-3, 1e-3, L, loss, bf16_points=("fact" if U + I <= R else "plain") if level == 2 else None)
    assert abs(la - want_loss) <= (1e-4 if level == 2 else 1e-5) * abs(want_loss)


@pytest.mark.parametrize("model,loss,B,L,d", [("NeuMF", 0, 256, 2, 24), ("NeuMF", 3, 1000, 3, 16), ("GMF", 0, 100, 2, 8), ("MLP", 2, 37, 1, 12),
                                              ("NeuMF", 0, 2000, 2, 24), ("MLP", 3, 4096, 2, 16), ("GMF", 1, 700, 1, 8), ("NeuMF", 0, 4000, 2, 16), ("GMF", 3, 8192, 1, 8)])
def test_neumf_small_steps_scatter_in_one_launch(model, loss, B, L, d, monkeypatch):
    """Round 6: at most 1024 rows per step (the reference's batch of 256 samples is 512) - the embedding gradients come from
    one launch (k_nmf_scatter_scan: every row's key compared with all keys, the first occurrence owns the table row; its
    predecessor k_nmf_scatter_small sorted the rows in LDS - bit-identical) instead of ~22 launches.  Against the
    owner-based scatter it replaces (DAISY_NMF_SCATTER_SMALL=0; other association of the same sums: fp32 round-off) and the
    fp64 oracle; hot rows (7 users), every model variant, point-wise rows, a row count that is no power of two; repeatable."""
    from daisyrec_amd import ops
    rng = np.random.default_rng(B + d)
    U, I = 7, 300
    dm = d << (L - 1)
    shapes = {"uG": (U, d), "iG": (I, d), "uM": (U, dm), "iM": (I, dm), "Wp": (1, d if model != "NeuMF" else 2 * d), "bp": (1,)}
    w = 2 * dm
    for l in range(1, L + 1):
        shapes[f"W{l}"], shapes[f"b{l}"] = (w // 2, w), (w // 2,)
        w //= 2
    p_np = {k: (rng.standard_normal(s) * 0.2).astype(np.float32) for k, s in shapes.items()}
    u, i = (rng.integers(0, n, B).astype(np.int32) for n in (U, I))
    j = (rng.integers(0, I, B) if loss < 3 else rng.integers(0, 2, B)).astype(np.int32)
    R = B if loss >= 3 else 2 * B
    idx = [torch.as_tensor(x).to(DEV) for x in (u, i, j)]

    def run(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        p = _dev(p_np)
        grads = {k: torch.zeros_like(v) for k, v in p.items()}
        ctx = ops.NeumfContext(R, d, L, U, I, model=model)
        ctx.step_grads(p, grads, *idx, loss, 1e-3, 2e-3)
        out = float(ctx.stats[11].cpu()), {k: v.cpu().numpy() for k, v in grads.items()}
        ctx.close()
        return out

    la, ga = run({"DAISY_NMF_SCATTER_SMALL": "1"})
    la2, ga2 = run({"DAISY_NMF_SCATTER_SMALL": "1"})
    # the sorting kernel the scanning one replaced: same sums, same order (it takes 1024 rows; beyond, mode 2 is the scan again)
    ls, gs = run({"DAISY_NMF_SCATTER_SMALL": "2"})
    lb, gb = run({"DAISY_NMF_SCATTER_SMALL": "0"})
    want_loss, want = NO.neumf_grad(p_np, u, i, j, 1e-3, 2e-3, L, loss, model)
    assert la == la2 == lb == ls and abs(la - want_loss) <= 1e-5 * abs(want_loss)
    for k in ("uG", "iG", "uM", "iM"):
        assert np.array_equal(ga[k], ga2[k]) and np.array_equal(ga[k], gs[k]), k
        tol = 3e-4 * np.abs(want[k]).max() + 3e-6 * (1 + np.sqrt(R))
        assert np.abs(ga[k] - want[k]).max() <= tol and np.abs(ga[k] - gb[k]).max() <= tol, (k, float(np.abs(ga[k] - want[k]).max()), tol)


@pytest.mark.parametrize("loss,B,L,d,pdrop", [(0, 256, 2, 24, 0.5), (0, 250, 2, 24, 0.0), (3, 1000, 3, 16, 0.3), (2, 37, 1, 12, 0.0),
                                              (4, 512, 2, 32, 0.0), (1, 7, 3, 8, 0.5), (0, 2048, 2, 24, 0.5), (3, 3001, 2, 16, 0.0),
                                              (0, 1100, 3, 16, 0.2), (0, 4096, 2, 24, 0.5), (3, 8000, 2, 16, 0.0)])
def test_neumf_small_steps_between_gather_and_scatter_in_one_launch(loss, B, L, d, pdrop, monkeypatch):
    """Round 6: steps of at most 8192 rows in the fp32 mode run the gather, every layer, the predict layer, the criterion and their backward
    pass in one launch with the weights in LDS (csrc/neumf_mid.hip: k_nmf_mid + the fixed-order sum of its workgroups' slabs)
    instead of 17 launches.  Against the fp64 oracle under the same dropout masks and against the layer-by-layer kernels it
    replaces (DAISY_NMF_MID=0: other association of the same fp32 sums); every criterion, ragged batches (250, 37, 7 samples:
    workgroups with rows past the batch), point-wise rows; repeatable to the bit."""
    from daisyrec_amd import ops
    rng = np.random.default_rng(B + d)
    U, I, seed = 90, 300, 1234
    dm = d << (L - 1)
    shapes = {"uG": (U, d), "iG": (I, d), "uM": (U, dm), "iM": (I, dm), "Wp": (1, 2 * d), "bp": (1,)}
    w = 2 * dm
    for l in range(1, L + 1):
        shapes[f"W{l}"], shapes[f"b{l}"] = (w // 2, w), (w // 2,)
        w //= 2
    p_np = {k: (rng.standard_normal(s) * 0.25).astype(np.float32) for k, s in shapes.items()}
    u, i = (rng.integers(0, n, B).astype(np.int32) for n in (U, I))
    j = (rng.integers(0, I, B) if loss < 3 else rng.integers(0, 2, B)).astype(np.int32)
    R = B if loss >= 3 else 2 * B
    idx = [torch.as_tensor(x).to(DEV) for x in (u, i, j)]

    def run(mid):
        monkeypatch.setenv("DAISY_NMF_MID", mid)
        p = _dev(p_np)
        grads = {k: torch.zeros_like(v) for k, v in p.items()}
        ctx = ops.NeumfContext(R, d, L, U, I, model="NeuMF")
        ctx.step_grads(p, grads, *idx, loss, 1e-3, 2e-3, dropout=pdrop, seed=seed)
        out = float(ctx.stats[11].cpu()), {k: v.cpu().numpy() for k, v in grads.items()}
        ctx.close()
        return out

    la, ga = run("1")
    la2, ga2 = run("1")
    lb, gb = run("0")
    masks = {}
    if pdrop:
        masks = {"masks_pos": NO.dropout_masks(seed, np.arange(B), d, L, pdrop)}
        if loss < 3:
            masks["masks_neg"] = NO.dropout_masks(seed, np.arange(B, 2 * B), d, L, pdrop)
    want_loss, want = NO.neumf_grad(p_np, u, i, j, 1e-3, 2e-3, L, loss, "NeuMF", **masks)
    assert la == la2
    assert abs(la - want_loss) <= 1e-5 * abs(want_loss) and abs(la - lb) <= 1e-5 * abs(want_loss)
    assert any(not np.array_equal(ga[k], gb[k]) for k in shapes)          # the one-launch path really ran (other summation order)
    for k in shapes:
        assert np.array_equal(ga[k], ga2[k]), k
        tol = 3e-4 * np.abs(want[k]).max() + 3e-6 * (1 + np.sqrt(R))
        assert np.abs(ga[k] - want[k]).max() <= tol and np.abs(ga[k] - gb[k]).max() <= tol, (
            k, float(np.abs(ga[k] - want[k]).max()), float(np.abs(ga[k] - gb[k]).max()), tol)


@pytest.mark.parametrize("opt,B,pdrop", [("adam", 256, 0.5), ("sgd", 100, 0.0), ("adagrad", 64, 0.2), ("rmsprop", 300, 0.0)])
def test_neumf_epoch_issued_by_the_library_equals_the_per_step_calls(opt, B, pdrop):
    """daisy_neumf_fit_epoch (the reference's loop over an epoch's batches, issued from the library) against the same steps
    called one by one - step_grads + the dense optimiser: identical parameters, optimiser state and epoch loss, a ragged
    last batch included."""
    from daisyrec_amd import ops
    from daisyrec_amd import _native as N
    rng = np.random.default_rng(11)
    U, I, d, L, n, seed = 120, 90, 16, 2, 1000, 5
    shapes = _tower_shapes(U, I, d, L)
    shapes["bp"] = shapes.pop("bp")          # (the one-element bias last, like the recommender's flat buffer: every view 16-byte aligned)
    sizes = {k: int(np.prod(v)) for k, v in shapes.items()}
    flat0 = (rng.standard_normal(sum(sizes.values())) * 0.2).astype(np.float32)
    tri = [torch.as_tensor(rng.integers(0, m, n).astype(np.int32)).to(DEV) for m in (U, I, I)]

    def views(flat):
        out, o = {}, 0
        for k, shp in shapes.items():
            out[k] = flat[o:o + sizes[k]].view(*shp)
            o += sizes[k]
        return out

    def run(native):
        W = torch.as_tensor(flat0).to(DEV).clone()
        g = torch.zeros_like(W)
        p, gr = views(W), views(g)
        optim = ops.DenseOptimizer(opt, 1e-2)
        ctx = ops.NeumfContext(2 * B, d, L, U, I)
        if native:
            steps = ctx.fit_epoch(p, gr, *tri, B, optim, W, g, 0, 1e-3, 2e-3, dropout=pdrop, seed_hi=seed << 32, step0=0)
        else:
            steps = 0
            for s0 in range(0, n, B):
                steps += 1
                ctx.step_grads(p, gr, *(t[s0:s0 + B] for t in tri), 0, 1e-3, 2e-3, dropout=pdrop, seed=(seed << 32) | steps)
                optim.next_step()
                optim.step(W, g)
        loss = float(ctx.stats[N.NST_LOSS_SUM].cpu())
        st = [t.cpu().numpy() for t in optim.state_for(W)]
        ctx.close()
        return steps, optim.t, loss, W.cpu().numpy(), st

    a, b = run(True), run(False)
    assert a[0] == b[0] == (n + B - 1) // B and a[1] == b[1] == a[0]
    assert a[2] == b[2] and np.isfinite(a[2]) and a[2] > 0
    assert np.array_equal(a[3], b[3]) and not np.array_equal(a[3], flat0)
    assert len(a[4]) == len(b[4]) and all(np.array_equal(x, y) for x, y in zip(a[4], b[4]))


@pytest.mark.parametrize("M,N,K,chunk", [(256, 512, 4096, 2048), (128, 64, 96, 32), (512, 256, 16384, 2048),
                                          (128, 128, 640, 64), (256, 64, 1024, 1024)])
def test_mfma_gemm_tn_bf16_weight_gradient_layout(M, N, K, chunk):
    """gW = dZ^T X with both operands stored [K][rows] as bf16: the fragments come out of the transposing LDS read
    (ds_read_b64_tr_b16).  Against the exact product of the bf16 operands; k slices that are (16384/2048 = 8) and
    are not a multiple of the 8 XCDs (the tile order differs), one and several tiles per slice."""
    from daisyrec_amd import ops
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    At = torch.randn(K, M, device=DEV, generator=g).to(torch.bfloat16)
    Bt = torch.randn(K, N, device=DEV, generator=g).to(torch.bfloat16)
    got = ops.gemm_tn_bf16(At, Bt, k_chunk=chunk).double().cpu()
    want = At.double().cpu().T @ Bt.double().cpu()
    assert (got - want).abs().max() <= 2e-5 * float(K) ** 0.5 * 4 + 1e-6 * want.abs().max()
    with pytest.raises(ValueError, match="gemm_tn_bf16"):
        ops.gemm_tn_bf16(At[:, :100].contiguous(), Bt)


@pytest.mark.parametrize("M,N,K", [(256, 128, 64), (384, 64, 512), (128, 256, 32), (1024, 256, 512), (2048, 128, 64)])
def test_mfma_gemm_bf16_storage(M, N, K):
    """all-bf16-operand GEMM of precision level 2: exact product of the stored bf16 values, fp32 accumulation,
    result rounded to bf16"""
    from daisyrec_amd import ops
    g = torch.Generator(device=DEV)
    g.manual_seed(M + N + K)
    A = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    Bm = (torch.randn(N, K, device=DEV, generator=g) * torch.linspace(0.1, 2.0, N, device=DEV)[:, None]).to(torch.bfloat16)
    got = ops.gemm_nt_bf16(A, Bm)
    exact = A.double() @ Bm.double().T
    assert got.dtype == torch.bfloat16 and got.shape == (M, N)
    assert float((got.double() - exact).abs().max()) <= 1e-2 * float(exact.abs().max())
    with pytest.raises(ValueError):
        ops.gemm_nt_bf16(A[:100].contiguous(), Bm)                         # partial row tile


def test_neumf_bf16_storage_dropout_and_eval():
    """level 2 with dropout (masks are functions of (seed, layer, row, column), so the fp32 run of the same seed
    drops the same elements) and through the scoring entry point"""
    from daisyrec_amd import ops
    rng = np.random.default_rng(9)
    U, I, d, L, B = 200, 150, 64, 2, 256
    dm = d << (L - 1)
    shapes = {"uG": (U, d), "iG": (I, d), "uM": (U, dm), "iM": (I, dm), "Wp": (1, 2 * d), "bp": (1,)}
    w = 2 * dm
    for l in range(1, L + 1):
        shapes[f"W{l}"], shapes[f"b{l}"] = (w // 2, w), (w // 2,)
        w //= 2
    p_np = {k: (rng.standard_normal(s) * 0.05).astype(np.float32) for k, s in shapes.items()}
    u, i, j = (torch.as_tensor(rng.integers(0, n, B).astype(np.int32)).to(DEV) for n in (U, I, I))
    out = []
    for level in (0, 2):
        p = _dev(p_np)
        grads = {k: torch.zeros_like(v) for k, v in p.items()}
        ctx = ops.NeumfContext(2 * B, d, L, U, I)
        ctx.set_precision(level)
        ctx.step_grads(p, grads, u, i, j, 0, 0.0, 0.0, dropout=0.5, seed=77)
        scores = ctx.scores(p, u.long(), i.long())
        out.append((float(ctx.stats[11].cpu()), grads["W1"].cpu().numpy(), scores.cpu().numpy()))
        ctx.close()
    assert abs(out[1][0] - out[0][0]) <= 5e-3 * abs(out[0][0])
    cos = float((out[0][1] * out[1][1]).sum() / (np.linalg.norm(out[0][1]) * np.linalg.norm(out[1][1])))
    assert cos > 0.97
    assert np.abs(out[0][2] - out[1][2]).max() <= 2e-2 * max(1e-3, np.abs(out[0][2]).max())


def test_neumf_argument_errors():
    from daisyrec_amd import ops
    with pytest.raises(ValueError):
        ops.NeumfContext(64, 6, 2, 10, 10)                      # factors must be a multiple of 4
    with pytest.raises(ValueError):
        ops.NeumfContext(64, 8, 9, 10, 10)                      # too many layers
    with pytest.raises(NotImplementedError):
        ops.NeumfContext(64, 8, 2, 10, 10, model="NeuMF-x")
    ctx = ops.NeumfContext(8, 8, 2, 10, 10)
    shapes = {"uG": (10, 8), "iG": (10, 8), "uM": (10, 16), "iM": (10, 16), "W1": (16, 32), "b1": (16,),
              "W2": (8, 16), "b2": (8,), "Wp": (1, 16), "bp": (1,)}
    p = {k: torch.zeros(s, device=DEV) for k, s in shapes.items()}
    g = {k: torch.zeros(s, device=DEV) for k, s in shapes.items()}
    idx = torch.zeros(8, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):                             # 2*8 rows > the context's 8
        ctx.step_grads(p, g, idx, idx, idx)
    with pytest.raises(NotImplementedError):                    # unknown loss id -> the reference's exception type
        ctx.step_grads(p, g, idx[:4], idx[:4], idx[:4], loss_type=9)
    with pytest.raises(ValueError):
        ctx.step_grads(p, g, idx[:4], idx[:4], idx[:4], dropout=1.0)
    with pytest.raises(TypeError):                              # host tensor / wrong dtype are refused, no CPU fallback
        ctx.step_grads(p, g, idx[:4].long(), idx[:4], idx[:4])
    ctx.close()


@pytest.mark.parametrize("level", [0, 2])
def test_neumf_step_is_bitwise_reproducible(level):
    """Hot users and items (every table row hit hundreds of times per step): the embedding gradients are
    segmented reductions on a single owner per row, so two runs give identical bits (fp32 atomics, which the first
    version of the scatter used, do not), and the sums agree with the fp64 oracle's to round-off - checked through the oracle
    KATs of this file, which run on the owner kernels.
    Round 3: the reductions over the batch rows that used fp32 atomics - the split-K slices of the MLP weight
    gradients (8 slices here), the bias column sums, the predict layer's gradient - now add per-workgroup partial
    sums in a fixed order (k_reduce_slices), so EVERY gradient of the step is bitwise repeatable."""
    from daisyrec_amd import ops
    rng = np.random.default_rng(21)
    U, I, d, L, B = 40, 30, 64, 2, 8192
    dm = d << (L - 1)
    shapes = {"uG": (U, d), "iG": (I, d), "uM": (U, dm), "iM": (I, dm), "Wp": (1, 2 * d), "bp": (1,)}
    w = 2 * dm
    for l in range(1, L + 1):
        shapes[f"W{l}"], shapes[f"b{l}"] = (w // 2, w), (w // 2,)
        w //= 2
    p_np = {k: (rng.standard_normal(s) * 0.05).astype(np.float32) for k, s in shapes.items()}
    u, i, j = (torch.as_tensor(rng.integers(0, n, B).astype(np.int32)).to(DEV) for n in (U, I, I))
    outs = []
    for _ in range(2):
        p = _dev(p_np)
        grads = {k: torch.zeros_like(v) for k, v in p.items()}
        ctx = ops.NeumfContext(2 * B, d, L, U, I)
        ctx.set_precision(level)
        for step in range(2):                      # the second call accumulates on top of the first (contract)
            ctx.step_grads(p, grads, u, i, j, 0, 1e-3, 1e-3)
        outs.append({k: grads[k].cpu().numpy() for k in grads})
        ctx.close()
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
        if k != "bp":                              # (the predict bias has an exactly zero gradient under BPR, like autograd)
            assert np.abs(outs[0][k]).max() > 0, k


@pytest.mark.parametrize("loss,B", [(0, 256), (3, 512)])
def test_neumf_first_layer_through_the_tables(loss, B, monkeypatch):
    """Round 5 (precision level 2, dropout 0, fewer distinct table rows than rows in the step): the MLP's first layer
    factored through the embedding tables - x1 = relu(T_u[user] + T_i[item] + b1) with T = table x W1[:, half]^T, and in the
    backward pass gW1 / the MLP tables' gradients from the segmented sums of dZ1 - against the plain bf16-storage path
    (DAISY_NMF_FACT=0) and the fp32 parity mode: the same step up to bf16 rounding (the factored path rounds LESS: its
    first layer runs on the fp32 tables), every parameter's gradient, the loss, bitwise repeatable."""
    from daisyrec_amd import ops
    rng = np.random.default_rng(15)
    U, I, d, L = 100, 80, 64, 3
    dm = d << (L - 1)
    shapes = {"uG": (U, d), "iG": (I, d), "uM": (U, dm), "iM": (I, dm), "Wp": (1, 2 * d), "bp": (1,)}
    w = 2 * dm
    for l in range(1, L + 1):
        shapes[f"W{l}"], shapes[f"b{l}"] = (w // 2, w), (w // 2,)
        w //= 2
    p_np = {k: (rng.standard_normal(s) * 0.05).astype(np.float32) for k, s in shapes.items()}
    u, i = (torch.as_tensor(rng.integers(0, n, B).astype(np.int32)).to(DEV) for n in (U, I))
    j = torch.as_tensor((rng.integers(0, I, B) if loss == 0 else rng.integers(0, 2, B)).astype(np.int32)).to(DEV)
    R = B if loss >= 3 else 2 * B
    assert U + I <= R

    def run(level, fact):
        monkeypatch.setenv("DAISY_NMF_FACT", fact)
        p = _dev(p_np)
        grads = {k: torch.zeros_like(v) for k, v in p.items()}
        ctx = ops.NeumfContext(R, d, L, U, I)
        ctx.set_precision(level)
        ctx.step_grads(p, grads, u, i, j, loss, 1e-3, 1e-3)
        out = float(ctx.stats[11].cpu()), {k: v.cpu().numpy() for k, v in grads.items()}
        ctx.close()
        return out

    l32, g32 = run(0, "1")
    lf, gf = run(2, "1")
    lp, gp = run(2, "0")
    lf2, gf2 = run(2, "1")
    assert lf == lf2 and all(np.array_equal(gf[k], gf2[k]) for k in shapes)          # reproducible
    assert lf != lp                                                                 # the factored path really ran
    assert abs(lf - l32) <= 2e-3 * abs(l32) and abs(lp - l32) <= 2e-3 * abs(l32)
    for k in shapes:
        n32 = np.linalg.norm(g32[k])
        if n32 == 0:
            continue
        ef = np.linalg.norm(gf[k] - g32[k]) / n32
        ep = np.linalg.norm(gp[k] - g32[k]) / n32
        cos = float((gf[k] * g32[k]).sum() / (np.linalg.norm(gf[k]) * n32 + 1e-30))
        assert ef < 0.25 and cos > 0.97, (k, ef, ep, cos)     # (against the FP32 mode: bf16's own distance from it; the tight
        assert ef < 2.5 * ep + 0.03, (k, ef, ep)             # check is test_neumf_bf16_step_against_the_bf16_oracle above)


# (level, d, L, U, I, max_rows, [(call, B or pairs, dropout)]): the calls one context serves, and the path each of them takes
REUSE_SEQUENCES = {
    "fp32": (0, 24, 2, 60, 50, 8400, [("step", 256, 0.0),        # the one-launch mid kernel + the scanning scatter
                                       ("step", 4200, 0.0),       # first layer through the tables, owner chain, counting pass
                                       ("scores", 500, 0.0),      # eval forward
                                       ("step", 4200, 0.3),       # plain layered path, counting pass
                                       ("step", 256, 0.0)]),      # mid + scan again
    "bf16": (2, 64, 3, 40, 30, 4224, [("step", 256, 0.0),         # fused tower, radix-sort owner chain
                                       ("step", 100, 0.0),        # 200 rows, not whole tiles: level 1, plain + scanning scatter
                                       ("step", 2112, 0.0),       # tower + counting pass
                                       ("step", 256, 0.0)]),      # tower + radix sorts again
}


@pytest.mark.parametrize("name", sorted(REUSE_SEQUENCES))
def test_neumf_context_reused_across_paths(name, monkeypatch):
    """One context serves a sequence of calls that take different paths (REUSE_SEQUENCES: the paths follow from neumf_path and
    neumf_scatter at the default settings).  Every call's loss and every gradient - the scores of the eval call - must equal
    BIT FOR BIT what a fresh context of the same max_rows (the workspace size feeds the split-K slice length, hence the
    summation order) produces for that call alone: nothing a call decides or leaves behind - its path, the table products,
    the count and row-sum tables the scatter keeps all-zero between calls - may reach the next one."""
    from daisyrec_amd import ops
    for var in ("DAISY_NMF_MID", "DAISY_NMF_FACT", "DAISY_NMF_TOWER", "DAISY_NMF_COUNTING", "DAISY_NMF_SCATTER_SMALL"):
        monkeypatch.delenv(var, raising=False)
    level, d, L, U, I, max_rows, calls = REUSE_SEQUENCES[name]
    rng = np.random.default_rng(3 + d)
    shapes = _tower_shapes(U, I, d, L)
    p = _dev({k: (rng.standard_normal(s) * 0.1).astype(np.float32) for k, s in shapes.items()})
    batches = [[torch.as_tensor(rng.integers(0, m, n).astype(np.int32)).to(DEV) for m in (U, I, I)] for _, n, _ in calls]

    def context():
        ctx = ops.NeumfContext(max_rows, d, L, U, I)
        ctx.set_precision(level)
        return ctx

    def call(ctx, k):
        kind, _, pdrop = calls[k]
        u, i, j = batches[k]
        if kind == "scores":
            return {"scores": ctx.scores(p, u.long(), i.long()).cpu().numpy()}
        grads = {key: torch.zeros_like(v) for key, v in p.items()}
        ctx.step_grads(p, grads, u, i, j, 0, 1e-3, 1e-3, dropout=pdrop, seed=99)
        return {"loss": ctx.stats[11].cpu().numpy(), **{key: v.cpu().numpy() for key, v in grads.items()}}

    shared = context()
    for k in range(len(calls)):
        got = call(shared, k)
        fresh = context()
        want = call(fresh, k)
        fresh.close()
        for key in want:
            assert np.array_equal(got[key], want[key]), (name, k, calls[k], key)
        if calls[k][0] == "step":
            assert np.isfinite(want["loss"]) and all(np.abs(want[key]).max() > 0 for key in ("uG", "iM", "W1", "Wp")), (name, k)
    shared.close()
