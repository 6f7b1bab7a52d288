"""NGCF on the GPU: the layer kernels against the float64 oracle (tests/ngcf_oracle.py, gradients by torch autograd),
the dropout masks, and the model against the golden vectors of the REAL reference NGCF (tests/golden/kat_ngcf.npz)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import ngcf_oracle as NO
from conftest import mf_config
from test_oracle_neumf import assert_params_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(HERE, "golden", "kat_ngcf.npz"))


def _t(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _layer_inputs(rng, n, di, do):
    E = rng.standard_normal((n, di)).astype(np.float32)
    X = rng.standard_normal((n, di)).astype(np.float32)
    W1 = (rng.standard_normal((do, di)) / np.sqrt(di)).astype(np.float32)
    W2 = (rng.standard_normal((do, di)) / np.sqrt(di)).astype(np.float32)
    b1 = (rng.standard_normal(do) * 0.1).astype(np.float32)
    b2 = -b1                                      # b1 + b2 = 0: rows with E = X = 0 have Z = 0 and norm 0
    zero = rng.choice(n, size=max(1, n // 50), replace=False) if n > 1 else np.array([], np.int64)
    E[zero] = 0
    X[zero] = 0
    dY = rng.standard_normal((n, do)).astype(np.float32)
    return E, X, W1, b1, W2, b2, dY, zero


def _run_layer(E, X, W1, b1, W2, b2, dY, mess_p=0.0, seed=0, layer=0, pitch_pad=3):
    """forward + backward + reduce on the device with E and Y as column slices of wider buffers"""
    from daisyrec_amd import ops
    n, di = E.shape
    do = W1.shape[0]
    cat = torch.full((n, di + do + pitch_pad), float("nan"), device=DEV)
    cat[:, :di] = _t(E)
    Es, Ys = cat[:, :di], cat[:, di:di + do]
    Xd, norm = _t(X), torch.empty(n, device=DEV)
    W = [_t(w) for w in (W1, b1, W2, b2)]
    ops.ngcf_layer_forward(Es, Xd, *W, Ys, norm, mess_p, seed, layer)
    dE, dX = torch.empty(n, di, device=DEV), torch.empty(n, di, device=DEV)
    ws = torch.empty(ops.ngcf_ws_bytes(n, di, do), dtype=torch.uint8, device=DEV)
    g = [torch.zeros_like(w) for w in W]
    ops.ngcf_layer_backward(_t(dY), Ys, norm, Es, Xd, W[0], W[2], dE, dX, ws, mess_p, seed, layer)
    ops.ngcf_wgrad_reduce(ws, n, di, do, g[0], g[1], g[2], g[3])
    torch.cuda.synchronize()
    assert not torch.isnan(cat[:, :di + do]).any()
    assert torch.isnan(cat[:, di + do:]).all()                   # nothing written past the slice
    return _np(Ys), _np(norm), _np(dE), _np(dX), [_np(x) for x in g]


def _rel(got, want):
    return np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)


SHAPES = [(36, 64), (64, 64), (64, 32), (20, 20), (100, 64), (256, 256)]


@pytest.mark.parametrize("di,do", SHAPES)
@pytest.mark.parametrize("n", [1, 63, 64, 50000])
def test_layer_forward_and_backward_vs_oracle(di, do, n):
    rng = np.random.default_rng(di * 1000 + do + n)
    E, X, W1, b1, W2, b2, dY, zero = _layer_inputs(rng, n, di, do)
    Y, norm, dE, dX, g = _run_layer(E, X, W1, b1, W2, b2, dY)
    Yr, nr, gr = NO.dense_layer_grads(E, X, W1, b1, W2, b2, dY)
    # the error of an fp32 K = 2 d_in dot product scales with sum |a b|, Y with 1 / |Z|: per-row allowance
    S, T = (E + X).astype(np.float64), (X * E).astype(np.float64)
    absz = np.abs(S) @ np.abs(W1.T).astype(np.float64) + np.abs(T) @ np.abs(W2.T).astype(np.float64) + 2 * np.abs(b1)
    Z = S @ W1.T + T @ W2.T
    zn = np.linalg.norm(np.where(Z > 0, Z, 0.2 * Z), axis=1)
    scale = np.maximum(1.0, np.linalg.norm(absz, axis=1) / np.maximum(zn, 1e-30))
    err = np.abs(Y - Yr).max(axis=1)
    assert (err <= 2e-6 * scale).all(), (err / scale).max()
    np.testing.assert_allclose(norm, nr, rtol=2e-6 * scale.max(), atol=1e-6)
    if len(zero):
        assert (norm[zero] == 0).all() and (Y[zero] == 0).all()
    for name, got in (("E", dE), ("X", dX), ("W1", g[0]), ("b1", g[1]), ("W2", g[2]), ("b2", g[3])):
        assert _rel(got, gr[name]) <= 1e-5, (name, _rel(got, gr[name]))
    if n >= 64:
        _, _, dE2, dX2, g2 = _run_layer(E, X, W1, b1, W2, b2, dY)
        for a, b in zip(g + [dE, dX], g2 + [dE2, dX2]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))      # bitwise repeatable


def test_torch_ops_layer_fwd_bwd_match_the_ctypes_path():
    import daisyrec_amd.torch_ops  # noqa: F401
    rng = np.random.default_rng(5)
    E, X, W1, b1, W2, b2, dY, _ = _layer_inputs(rng, 777, 36, 64)
    Y, norm, dE, dX, g = _run_layer(E, X, W1, b1, W2, b2, dY, mess_p=0.1, seed=9, layer=1)
    Yt, nt = torch.ops.daisyrec.ngcf_layer_fwd(_t(E), _t(X), _t(W1), _t(b1), _t(W2), _t(b2), 0.1, 9, 1)
    out = torch.ops.daisyrec.ngcf_layer_bwd(_t(dY), Yt, nt, _t(E), _t(X), _t(W1), _t(W2), 0.1, 9, 1)
    assert np.array_equal(_np(Yt), Y) and np.array_equal(_np(nt), norm)
    for a, b in zip(out, [dE, dX] + g):
        assert np.array_equal(_np(a), b)


def _graph(rng, U, I, n):
    from daisyrec_amd import ops
    gu, gi = rng.integers(0, U, n), rng.integers(0, I, n)
    return gu, gi, ops.LgcnGraph(_t(gu), _t(gi), U, I)


def test_dropout_masks_statistics_and_layer_with_dropout():
    from daisyrec_amd import ops
    rng = np.random.default_rng(11)
    n, p = 1_000_003, 0.3
    keep = _np(ops.dropout_mask(123, ops.NGCF_NODE_STREAM, n, p)).astype(bool)
    k, mu, sd = keep.sum(), n * (1 - p), np.sqrt(n * p * (1 - p))
    assert abs(k - mu) <= 5 * sd, (k, mu, sd)
    other = _np(ops.dropout_mask(124, ops.NGCF_NODE_STREAM, n, p)).astype(bool)
    assert 0.5 < (keep == other).mean() < 0.7                    # another seed: an independent mask
    assert _np(ops.dropout_mask(1, 5, 100, 0.0)).all()
    # the layer with message dropout: the mask of the hook is the one the forward AND backward kernels use
    di, do, rows, mp, seed, layer = 36, 64, 3000, 0.2, 77, 2
    E, X, W1, b1, W2, b2, dY, _ = _layer_inputs(rng, rows, di, do)
    mk = _np(ops.dropout_mask(seed, ops.NGCF_MESS_STREAM + layer, rows * do, mp)).reshape(rows, do)
    Y, norm, dE, dX, g = _run_layer(E, X, W1, b1, W2, b2, dY, mp, seed, layer)
    Yr, nr, gr = NO.dense_layer_grads(E, X, W1, b1, W2, b2, dY, mess_keep=mk, mess_p=mp)
    assert ((Y == 0) >= (mk == 0)).all()
    assert np.abs(Y - Yr).max() <= 2e-5
    for name, got in (("E", dE), ("X", dX), ("W1", g[0]), ("b1", g[1]), ("W2", g[2]), ("b2", g[3])):
        assert _rel(got, gr[name]) <= 1e-5, name


@pytest.mark.parametrize("d", [64, 20, 7])
def test_masked_products_and_the_transpose(d):
    from daisyrec_amd import ops
    rng = np.random.default_rng(d)
    U, I = 300, 500
    gu, gi, graph = _graph(rng, U, I, 6000)
    N = U + I
    row, col, val = (_np(t) for t in graph.coo())
    p, seed = 0.3, 4242
    keep = _np(ops.dropout_mask(seed, ops.NGCF_NODE_STREAM, graph.nnz, p)).astype(bool)
    A = sp.csr_matrix((np.where(keep, val.astype(np.float64) / (1 - p), 0.0), (row, col)), shape=(N, N))
    wide = torch.randn(N, d + 5, device=DEV)
    x = wide[:, 2:2 + d]                                          # a column slice: pitch d + 5
    xn = _np(x).astype(np.float64)
    y = graph.spmm(x, pitch=d + 5, keep=(p, seed))
    np.testing.assert_allclose(_np(y), A @ xn, rtol=1e-5, atol=1e-6)
    yt = graph.spmm(x, keep=(p, seed), transpose=True, out=torch.zeros(N, d, device=DEV))
    np.testing.assert_allclose(_np(yt), A.T @ xn, rtol=1e-5, atol=1e-6)
    acc = torch.ones(N, d, device=DEV)
    graph.spmm(x, accumulate=True, out=acc)
    A0 = sp.csr_matrix((val.astype(np.float64), (row, col)), shape=(N, N))
    np.testing.assert_allclose(_np(acc), 1.0 + A0 @ xn, rtol=1e-5, atol=1e-6)
    # the unmasked strided product equals LightGCN's product, and repeats bit for bit
    a, b = graph.spmm(x, out=torch.empty(N, d, device=DEV)), graph.spmm(x.contiguous())
    np.testing.assert_allclose(_np(a), _np(b), rtol=1e-6, atol=1e-7)
    assert torch.equal(a, graph.spmm(x, out=torch.empty(N, d, device=DEV)))
    graph.close()


def _config(U, I, f, hidden, gu, gi, **over):
    cfg = mf_config(user_num=U, item_num=I, factors=f, algo_name="ngcf", hidden_size_list=hidden, node_dropout=0.0,
                    mess_dropout=0.0, reg_1=0.0, reg_2=0.0, lr=0.01,
                    inter_matrix=sp.coo_matrix((np.ones(len(gu), np.float32), (gu, gi)), shape=(U, I)))
    cfg.update(over)
    return cfg


def _params(g, prefix):
    p = f"{prefix}/p/"
    return {k[len(p):]: g[k] for k in g.files if k.startswith(p)}


def test_model_initial_parameters_and_keys_are_the_references(kat):
    from daisyrec_amd.model import NGCF
    g = kat
    for name in [str(x) for x in g["names"]]:
        U, I, f, B, ns, seed = (int(x) for x in g[f"{name}/meta"])
        torch.manual_seed(seed)
        model = NGCF(_config(U, I, f, [int(x) for x in g[f"{name}/hidden"]], g[f"{name}/gu"], g[f"{name}/gi"],
                             init_method="default", optimizer=str(g[f"{name}/optimizer"])))
        want = _params(g, f"{name}/init")
        sd = model.state_dict()
        assert list(sd.keys())[:2] == ["embed_user.weight", "embed_item.weight"] and set(sd) == set(want)
        for k, v in sd.items():
            assert np.array_equal(_np(v), want[k]), (name, k)
    assert list(model.state_dict().keys())[2] == "gnn_layers.0.linear.weight"


def test_model_step_kats(kat):
    from daisyrec_amd import ops
    from daisyrec_amd.model import NGCF
    g = kat
    for name in [str(x) for x in g["names"]]:
        U, I, f, B, ns, seed = (int(x) for x in g[f"{name}/meta"])
        lr, r1, r2 = (float(x) for x in g[f"{name}/hyper"])
        lt, opt = str(g[f"{name}/loss_type"]), str(g[f"{name}/optimizer"])
        torch.manual_seed(seed)
        model = NGCF(_config(U, I, f, [int(x) for x in g[f"{name}/hidden"]], g[f"{name}/gu"], g[f"{name}/gi"],
                             reg_1=r1, reg_2=r2, lr=lr, loss_type=lt, optimizer=opt))
        flat = model._params()
        loss_id = ops.loss_id(lt)
        ctx, ctx_ego = model._contexts(B, loss_id)
        optim = ops.DenseOptimizer(model.optimizer, lr)
        for s in range(ns):
            u, i, j = (_t(g[f"{name}/{k}"][s]) for k in "uij")
            model._batch_grads(ctx, ctx_ego, u, i, j, loss_id)
            loss, ref = float(ctx.stats[7].cpu()), float(g[f"{name}/loss"][s])
            assert abs(loss - ref) <= 1e-5 * abs(ref), (name, s, loss, ref)
            optim.next_step()
            optim.step(flat, model._gflat)
        got = {k: _np(v) for k, v in model.state_dict().items()}
        want = _params(g, f"{name}/final")
        assert_params_close(got, want, sorted(want), name, 5e-6, adam_lr=lr if model.optimizer == "adam" else None,
                            steps=ns, frac=0.98)
        ctx.close()
        ctx_ego.close()


def test_model_restore_rank_full_rank_predict(kat):
    from daisyrec_amd.model import NGCF
    from daisyrec_amd.utils.dataset import CandidatesDataset, get_dataloader
    g = kat
    U, I, f = (int(x) for x in g["rank/meta"])
    model = NGCF(_config(U, I, f, [int(x) for x in g["rank/hidden"]], g["rank/gu"], g["rank/gi"],
                         topk=int(g["rank/topk"])))
    with torch.no_grad():
        for k, v in model.state_dict().items():
            v.copy_(torch.from_numpy(g[f"rank/p/{k}"]))
    model.eval()
    us, cands = g["rank/us"], g["rank/cands"]
    loader = get_dataloader(CandidatesDataset([[int(us[b]), cands[b]] for b in range(len(us))]), batch_size=4,
                            shuffle=False, num_workers=0)
    preds = model.rank(loader)
    np.testing.assert_allclose(_np(model.restore_user_e), g["rank/restore_user"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(_np(model.restore_item_e), g["rank/restore_item"], rtol=1e-5, atol=1e-6)
    np.testing.assert_array_equal(preds, g["rank/preds"])
    full = np.stack([model.full_rank(int(u)) for u in us])
    np.testing.assert_array_equal(full, g["rank/full"])
    pr = np.array([model.predict(int(us[b]), int(cands[b, 0])) for b in range(len(us))], dtype=np.float32)
    np.testing.assert_allclose(pr, g["rank/predict"], rtol=1e-5, atol=1e-6)


def test_ml100k_first_50_batches(kat):
    """test.py --algo_name ngcf (ngcf.yaml, mess_dropout 0): one epoch over the reference's first 12 800 triples."""
    from daisyrec_amd.model import NGCF
    from daisyrec_amd.utils.dataset import BasicDataset, get_dataloader
    g = kat
    U, I, f = (int(x) for x in g["ml/meta"])
    lr, r1, r2 = (float(x) for x in g["ml/hyper"])
    torch.manual_seed(int(g["ml/seed"]))
    model = NGCF(_config(U, I, f, None, g["ml/train_users"], g["ml/train_items"], lr=lr, reg_1=r1, reg_2=r2, epochs=1,
                         seed=int(g["ml/seed"])))
    for k, v in model.state_dict().items():
        assert np.array_equal(_np(v), g[f"ml/init/p/{k}"]), k
    loader = get_dataloader(BasicDataset(g["ml/samples"]), batch_size=int(g["ml/batch_size"]), shuffle=True,
                            num_workers=0)
    torch.set_rng_state(torch.from_numpy(g["ml/rng_state_before_fit"]))
    model.fit(loader)
    ref = float(g["ml/epoch_losses"][0])
    assert abs(model.epoch_losses[0] - ref) <= 1e-5 * abs(ref), (model.epoch_losses, ref)
    assert abs(g["ml/batch_losses"].sum() - ref) <= 1e-6 * abs(ref)


def _small(rng, **over):
    from daisyrec_amd.model import NGCF
    U, I = 80, 120
    gu, gi = rng.integers(0, U, 1500), rng.integers(0, I, 1500)
    cfg = _config(U, I, 36, [64, 32], gu, gi, epochs=2, **over)
    return NGCF(cfg), U, I


def _loader(rng, U, I, n, B=128):
    from daisyrec_amd.utils.dataset import BasicDataset, get_dataloader
    t = np.stack([rng.integers(0, U, n), rng.integers(0, I, n), rng.integers(0, I, n)], 1).astype(np.int32)
    return get_dataloader(BasicDataset(t), batch_size=B, shuffle=True, num_workers=0)


def test_sorted_mode_is_bitwise_repeatable_with_dropout():
    runs = []
    for _ in range(2):
        torch.manual_seed(7)
        rng = np.random.default_rng(7)
        model, U, I = _small(rng, item_mode="sorted", node_dropout=0.3, mess_dropout=0.2, reg_1=1e-3, reg_2=1e-3)
        model.fit(_loader(rng, U, I, 1000))
        runs.append(({k: _np(v) for k, v in model.state_dict().items()}, list(model.epoch_losses)))
    assert runs[0][1] == runs[1][1]
    for k in runs[0][0]:
        assert np.array_equal(runs[0][0][k].view(np.uint32), runs[1][0][k].view(np.uint32)), k


def test_full_step_with_dropout_matches_the_oracle():
    """node_dropout 0.3 + mess_dropout 0.2: the masks read back through the hook, fed to the oracle"""
    from daisyrec_amd import ops
    rng = np.random.default_rng(3)
    torch.manual_seed(3)
    model, U, I = _small(rng, node_dropout=0.3, mess_dropout=0.2, reg_1=1e-3, reg_2=1e-3)
    model._params()
    p0 = {k: _np(v).copy() for k, v in model.state_dict().items()}
    B = 96
    u, i, j = rng.integers(0, U, B), rng.integers(0, I, B), rng.integers(0, I, B)
    loss_id = ops.loss_id("BPR")
    ctx, ctx_ego = model._contexts(B, loss_id)
    model.train()
    calls = model._calls
    model._batch_grads(ctx, ctx_ego, *(_t(x.astype(np.int32)) for x in (u, i, j)), loss_id)
    seed = (model._seed << 32) | (calls + 1)
    graph = model._adj()
    row, col, _ = (_np(t) for t in graph.coo())
    A = NO.adj(model.interaction_matrix.row, model.interaction_matrix.col, U, I)
    assert np.array_equal(A[1], col)                             # the device entry order is the oracle's CSR order
    node = _np(ops.dropout_mask(seed, ops.NGCF_NODE_STREAM, graph.nnz, 0.3)).astype(bool)
    w = model._widths
    mess = [_np(ops.dropout_mask(seed, ops.NGCF_MESS_STREAM + k, (U + I) * w[k + 1], 0.2)).reshape(U + I, w[k + 1])
            for k in range(len(w) - 1)]
    loss, grads = NO.loss_and_grads(A, p0, w, u, i, j, "BPR", 1e-3, 1e-3, node_keep=node, node_p=0.3, mess_keeps=mess,
                                    mess_p=0.2)
    got = float(ctx.stats[7].cpu())
    assert abs(got - loss) <= 1e-5 * abs(loss), (got, loss)
    for k, v in model._grads.items():
        assert _rel(_np(v).astype(np.float64), grads[k]) <= 1e-5, (k, _rel(_np(v), grads[k]))
    ctx.close()
    ctx_ego.close()


def test_eval_forward_keeps_message_dropout_and_drops_no_nodes():
    """the reference quirk: nn.Dropout built inside forward is in training mode, so eval-time embeddings are dropped"""
    rng = np.random.default_rng(1)
    model, U, I = _small(rng, mess_dropout=0.5, node_dropout=0.5)
    model.eval()
    ue, ie = model.forward()
    f = model.embedding_size
    zeros = (_np(torch.cat([ue, ie], 0))[:, f:] == 0).mean()
    assert 0.4 < zeros < 0.6                                     # about half of the propagated columns dropped
    model2, _, _ = _small(np.random.default_rng(1), mess_dropout=0.0, node_dropout=0.5)
    model2.eval()
    with torch.no_grad():
        for k, v in model2.state_dict().items():
            v.copy_(model.state_dict()[k])
    a = torch.cat(model2.forward(), 0)
    assert torch.equal(a, torch.cat(model2.forward(), 0))       # eval: no node dropout, no message dropout at p = 0


def test_zero_samples_hidden_default_and_invalid_loss():
    from daisyrec_amd.model import NGCF
    from daisyrec_amd.utils.dataset import BasicDataset, get_dataloader
    rng = np.random.default_rng(2)
    model, U, I = _small(rng)
    before = {k: _np(v).copy() for k, v in model.state_dict().items()}
    model.fit(get_dataloader(BasicDataset(np.zeros((0, 3), np.int32)), batch_size=64, shuffle=False, num_workers=0))
    assert model.epoch_losses == [0.0, 0.0]
    for k, v in model.state_dict().items():
        assert np.array_equal(_np(v), before[k])
    gu, gi = rng.integers(0, 30, 200), rng.integers(0, 40, 200)
    m = NGCF(_config(30, 40, 16, None, gu, gi))
    assert m.hidden_size_list == [16, 64, 64, 64]
    assert list(m.state_dict().keys())[-1] == "gnn_layers.2.interact_transform.bias"
    m.fit(_loader(rng, 30, 40, 300, B=64))
    assert len(m.epoch_losses) == 3 and all(np.isfinite(m.epoch_losses))
    bad = NGCF(_config(30, 40, 16, [8], gu, gi, loss_type="XYZ"))
    with pytest.raises(NotImplementedError):
        bad.fit(_loader(rng, 30, 40, 100))
    with pytest.raises(ValueError):
        NGCF(_config(30, 40, 16, [300], gu, gi))
