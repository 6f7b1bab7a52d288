"""Multi-VAE on the device (csrc/vae.hip through daisy_vae_*): the reference's step KATs with its recorded noise, the
ml-100k run of run_examples/test.py replayed batch by batch, bitwise repeatability, the device noise, the anneal
counter, eval / training-mode scoring, state_dict round trips, the torch op, and one large-catalogue step against the
float64 oracle.  Reads only tests/golden/ and seeded synthetic data."""
import os

import numpy as np
import pytest
import torch

import vae_oracle as VO
from test_oracle_vae import CASES, close, kat_model, kat_steps, vae_config

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(HERE, "golden", "kat_vae.npz"))


@pytest.fixture(scope="module")
def ml():
    return np.load(os.path.join(HERE, "golden", "kat_vae_ml100k.npz"))


def f32(x):
    return float(np.float32(x))


def replay(m, batches, optimizer, p, cap, total, update0=0):
    """daisy_vae_step_grads with the given noise + the dense optimiser per batch: [(users, keep, eps)] -> losses"""
    from daisyrec_amd import ops
    from daisyrec_amd import _native as N
    W = m._params()
    csr, lens = m._csr()
    B = max(len(b[0]) for b in batches)
    E = max(int(lens[torch.as_tensor(b[0])].sum()) for b in batches)
    ctx = ops.VaeContext(B, max(E, 1), m.item_num, m.layers, m.lat_dim)
    optim = ops.DenseOptimizer(optimizer, m.lr)
    g = torch.zeros_like(W)
    losses, update = [], update0
    for users, keep, eps in batches:
        users = torch.as_tensor(np.asarray(users), dtype=torch.int64)
        entries = int(lens[users].sum())
        assert keep.size == entries
        update += 1
        ctx.step_grads(W, g, csr, users.cuda(), entries, keep=torch.from_numpy(np.asarray(keep, np.uint8)).cuda(),
                       eps=torch.from_numpy(np.asarray(eps, np.float32)).cuda(), train=True, dropout=p,
                       anneal=f32(VO.anneal_at(update, cap, total)))
        losses.append(float(ctx.stats[N.VST_LOSS]))
        optim.next_step()
        optim.step(W, g)
    assert float(ctx.stats[N.VST_BAD_ROWS]) == 0
    ctx.close()
    return np.array(losses)


def host_state(m):
    return {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}


def rel_to_update(got, init, ref):
    """max |got - ref| over the parameter update ref - init, relative to the update's largest element"""
    upd_ref = np.asarray(ref, np.float64) - init
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(upd_ref).max(), 1e-30))


def grad_views(m, g):
    """the gradient buffer as tensors in the reference's layout (encoder.0.weight is stored item-major)"""
    out, off = {}, 0
    for name, p in m.named_parameters():
        n = p.numel()
        v = g[off:off + n]
        out[name] = v.view(p.shape[1], p.shape[0]).t() if name == "encoder.0.weight" else v.view(p.shape)
        off += n
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


# measured on the committed kernels: SGD updates ARE the gradient; the first steps of the adaptive
# optimisers are close to lr * sign(g), where gradient elements near 0 (sums that cancel) decide the sign
UPDATE_TOL = {"sgd": 1e-5, "adam": 2e-2, "adagrad": 2e-2, "rmsprop": 2e-2}


@pytest.mark.parametrize("case", CASES)
def test_step_kats_against_reference_and_oracle(kat, case):
    U, I, lat, B, ns, seed, total = (int(x) for x in kat[f"{case}/meta"])
    lr, p, cap = (float(x) for x in kat[f"{case}/hyper"])
    opt = str(kat[f"{case}/optimizer"])
    m = kat_model(kat, case)
    init = host_state(m)
    batches = [(kat[f"{case}/users"][k], kat[f"{case}/keep{k}"], kat[f"{case}/eps{k}"]) for k in range(ns)]
    losses = replay(m, batches, opt, p, cap, total)
    np.testing.assert_allclose(losses, kat[f"{case}/loss"], rtol=1e-5)
    ol, oparams = VO.run_steps(init, kat_steps(kat, case), lat, opt, lr, p, cap, total)
    np.testing.assert_allclose(losses, ol, rtol=1e-5)
    got = host_state(m)
    worst = {}
    for k, ref in oparams.items():
        worst[k] = rel_to_update(got[k], init[k], ref.numpy())
        assert worst[k] <= UPDATE_TOL[opt], (case, k, worst[k])
        # the reference's fp32 run against the same bound
        assert rel_to_update(kat[f"{case}/final/p/{k}"], init[k], ref.numpy()) <= UPDATE_TOL[opt], (case, k)
    print(case, "update error relative to each tensor's update (max over tensors):", max(worst.values()))


@pytest.mark.parametrize("case", CASES)
def test_step_gradients_against_oracle(kat, case):
    """the first step's gradient of every tensor against the float64 oracle, relative to the tensor's largest element"""
    from daisyrec_amd import ops
    U, I, lat, B, ns, seed, total = (int(x) for x in kat[f"{case}/meta"])
    lr, p, cap = (float(x) for x in kat[f"{case}/hyper"])
    m = kat_model(kat, case)
    init = host_state(m)
    W = m._params()
    csr, lens = m._csr()
    users = torch.from_numpy(kat[f"{case}/users"][0])
    E = int(lens[users].sum())
    ctx = ops.VaeContext(B, E, I, m.layers, lat)
    g = torch.zeros_like(W)
    an = f32(VO.anneal_at(1, cap, total))
    ctx.step_grads(W, g, csr, users.cuda(), E, keep=torch.from_numpy(kat[f"{case}/keep0"]).cuda(),
                   eps=torch.from_numpy(kat[f"{case}/eps0"]).cuda(), train=True, dropout=p, anneal=an)
    R, keep, eps = kat_steps(kat, case)[0]
    loss, og = VO.grads_of(init, R, lat, keep, eps, p, an)
    got = grad_views(m, g)
    for k, ref in og.items():
        err = np.abs(got[k] - ref).max() / max(np.abs(ref).max(), 1e-30)
        assert err <= 1e-5, (case, k, err)
    ctx.close()


def ml_model(ml, **over):
    """the mirror of test.py's model: the train split's histories, the reference's initial state"""
    from daisyrec_amd.model import VAECF
    U, I, lat, B, seed, total = (int(x) for x in ml["ml/meta"])
    lens = ml["ml/hist_len"].astype(np.int64)
    L = int(lens.max())
    hid = np.zeros((U, L), dtype=np.int64)
    hval = np.zeros((U, L), dtype=np.float32)
    pos = 0
    for u in range(U):
        hid[u, :lens[u]] = ml["ml/hist_items"][pos:pos + lens[u]]
        hval[u, :lens[u]] = 1.0
        pos += lens[u]
    torch.set_rng_state(torch.from_numpy(ml["ml/rng_state_before_model"]))
    cfg = dict(epochs=2)
    cfg.update(over)
    return VAECF(vae_config(user_num=U, item_num=I, history_item_id=torch.from_numpy(hid),
                            history_item_value=torch.from_numpy(hval), **cfg))


def test_ml100k_batches_and_rank_lists(ml):
    from daisyrec_amd import ops
    U, I, lat, B, seed, total = (int(x) for x in ml["ml/meta"])
    lr, p, cap = (float(x) for x in ml["ml/hyper"])
    m = ml_model(ml)
    nb = int(ml["ml/n_batches"])
    batches = [(ml[f"ml/users{k}"], np.unpackbits(ml[f"ml/keep{k}"])[:int(ml[f"ml/nkeep{k}"])], ml[f"ml/eps{k}"])
               for k in range(nb)]
    losses = replay(m, batches, "adam", p, cap, total)
    ref = ml["ml/batch_losses"]
    rel = np.abs(losses - ref) / np.abs(ref)
    print("ml-100k per-batch relative loss differences:", rel)
    assert rel[:2].max() <= 1e-5                            # the first batches
    assert rel.max() <= 1e-4                                # the whole 2-epoch run
    per = nb // 2
    np.testing.assert_allclose([losses[:per].sum(), losses[per:].sum()], ml["ml/epoch_losses"], rtol=1e-5)
    got = host_state(m)
    for k, v in got.items():
        if f"ml/final_idx/{k}" in ml:
            v = np.take(v, ml[f"ml/final_idx/{k}"], axis=1 if k == "encoder.0.weight" else 0)
        assert close(v, ml[f"ml/final/{k}"], 1e-4), (k, np.abs(v - ml[f"ml/final/{k}"]).max())
    # test.py's eval-mode rank lists of the first candidate users
    m.eval()
    users = torch.from_numpy(ml["ml/rank_users"])
    cands = torch.from_numpy(ml["ml/rank_cands"].astype(np.int64)).cuda()
    scores = m._scores(users, cands)
    lists = ops.topk_from_scores(scores, cands, m.topk).cpu().numpy()
    ref_lists = ml["ml/rank_preds"].astype(np.int64)
    # (candidates are drawn with replacement: a list may hold an item twice, so the lists compare as sets)
    overlap = np.mean([len(set(a) & set(b)) / len(set(b)) for a, b in zip(lists, ref_lists)])
    print("ml-100k rank-list overlap with the reference:", overlap)
    assert overlap >= 0.98


def test_two_seeded_fits_are_bitwise_equal_and_anneal_carries(ml):
    from torch.utils.data import DataLoader, Dataset

    class Users(Dataset):                                  # what AEDataset holds: the training users
        def __init__(self, data):
            self.data = data

        def __len__(self):
            return len(self.data)

        def __getitem__(self, k):
            return self.data[k]

    def run():
        m = ml_model(ml, seed=11)
        users = np.nonzero(ml["ml/hist_len"])[0]
        ds = Users(users)
        g = torch.Generator()
        g.manual_seed(5)
        loader = DataLoader(ds, batch_size=256, shuffle=True, generator=g)
        m.fit(loader)
        nb = (len(users) + 255) // 256
        assert m.update == 2 * nb and m._steps == 2 * nb
        first = {k: v.clone() for k, v in m.state_dict().items()}
        m.epochs = 1
        m.fit(loader)                                     # the counter carries on, Adam restarts
        assert m.update == 3 * nb
        return first, m.state_dict(), list(m.epoch_losses)
    a, a2, la = run()
    b, b2, lb = run()
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a2[k], b2[k]), k
    assert la == lb and all(np.isfinite(la))


def test_device_noise_statistics(ml):
    """the hash streams: the keep bits ARE daisy_dropout_mask's stream DAISY_VAE_KEEP_STREAM (a step with them passed
    explicitly gives the same bits), their kept fraction is about 1 - p, and eps is about N(0, 1)"""
    from daisyrec_amd import ops
    from daisyrec_amd import _native as N
    m = ml_model(ml)
    W = m._params()
    csr, lens = m._csr()
    users = torch.from_numpy(np.nonzero(ml["ml/hist_len"])[0][:256])
    E = int(lens[users].sum())
    ctx = ops.VaeContext(256, E, m.item_num, m.layers, m.lat_dim)
    g1, g2 = torch.zeros_like(W), torch.zeros_like(W)
    ctx.step_grads(W, g1, csr, users.cuda(), E, train=True, dropout=0.5, anneal=0.1, seed=123)
    l1 = float(ctx.stats[N.VST_LOSS])
    keep = ops.dropout_mask(123, N.VAE_KEEP_STREAM, E, 0.5)
    ctx.step_grads(W, g2, csr, users.cuda(), E, keep=keep, train=True, dropout=0.5, anneal=0.1, seed=123)
    assert float(ctx.stats[N.VST_LOSS]) == l1 and torch.equal(g1, g2)
    frac = float(keep.float().mean())
    assert abs(frac - 0.5) < 0.02, frac
    # eps: all weights 0, the decoder's first layer the identity, the last layer's first 64 rows unit vectors: mu = 0,
    # logvar = 0, so score[b][j] = tanh(eps[b][j]) for j < 64
    m2 = ml_model(ml, mlp_hidden_size=[64])
    W2 = m2._params()
    with torch.no_grad():
        W2.zero_()
        m2.decoder[0].weight.copy_(torch.eye(64))
        m2.decoder[2].weight[:64].copy_(torch.eye(64))
    ctx2 = ops.VaeContext(256, E, m2.item_num, m2.layers, m2.lat_dim)
    sc = ctx2.scores(W2, m2._csr()[0], users.cuda(), E, train=True, dropout=0.5, seed=99)
    eps = torch.atanh(sc[:, :64].double().clamp(-1 + 1e-7, 1 - 1e-7)).cpu()
    assert abs(float(eps.mean())) < 0.03 and abs(float(eps.var()) - 1.0) < 0.06, (float(eps.mean()), float(eps.var()))
    sc2 = ctx2.scores(W2, m2._csr()[0], users.cuda(), E, train=True, dropout=0.5, seed=99)
    assert torch.equal(sc, sc2)
    ctx.close()
    ctx2.close()


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_rank_full_rank_predict_against_reference(kat, mode):
    from daisyrec_amd.model import VAECF
    from daisyrec_amd import ops
    U, I, C, nB, topk, lat, ncalls = (int(x) for x in kat["rank/meta"])
    torch.manual_seed(3)
    m = VAECF(vae_config(user_num=U, item_num=I, mlp_hidden_size=[16], latent_dim=lat, topk=topk,
                         history_item_id=torch.from_numpy(kat["rank/hist_id"]),
                         history_item_value=torch.from_numpy(kat["rank/hist_val"])))
    m.load_state_dict({k[len("rank/params/p/"):]: torch.from_numpy(kat[k]) for k in kat.files
                       if k.startswith("rank/params/p/")})            # a reference-layout state dict
    us, cands = kat["rank/us"], kat["rank/cands"]
    if mode == "eval":
        m.eval()
        rk = []
        for b0 in range(0, nB, 4):
            rk.append(m.rank([(torch.from_numpy(us[b0:b0 + 4]), torch.from_numpy(cands[b0:b0 + 4]))]))
        np.testing.assert_array_equal(np.concatenate(rk), kat["rank/eval/preds"])
        np.testing.assert_array_equal(np.stack([m.full_rank(int(u)) for u in us]), kat["rank/eval/full"])
        pr = np.array([m.predict(int(us[b]), int(cands[b, 0])) for b in range(nB)], dtype=np.float32)
        np.testing.assert_allclose(pr, kat["rank/eval/predict"], rtol=1e-5, atol=1e-6)
        return
    m.train()
    out = []
    for k, b0 in enumerate(range(0, nB, 4)):
        cd = torch.from_numpy(cands[b0:b0 + 4]).cuda()
        sc = m._scores(torch.from_numpy(us[b0:b0 + 4]), cd, keep=torch.from_numpy(kat[f"rank/train/keep{k}"]).cuda(),
                       eps=torch.from_numpy(kat[f"rank/train/eps{k}"]).cuda())
        out.append(ops.topk_from_scores(sc, cd, topk).cpu().numpy())
    np.testing.assert_array_equal(np.concatenate(out).astype(np.float32), kat["rank/train/preds"])


def test_state_dict_layout_and_round_trip(kat):
    m = kat_model(kat, "vae_adam")
    before = host_state(m)
    m._params()                                               # moves into the flat buffer (encoder.0.weight item-major)
    sd = m.state_dict()
    assert list(sd) == list(before) and all(tuple(sd[k].shape) == before[k].shape for k in sd)
    for k in before:
        np.testing.assert_array_equal(sd[k].cpu().numpy(), before[k])
    assert [p.shape for p in m.parameters()][0] == torch.Size([16, int(kat["vae_adam/meta"][1])])
    m2 = kat_model(kat, "vae_adam")
    m2._params()
    with torch.no_grad():                                     # other values, same shapes
        for p in m2.parameters():
            p.mul_(0.5).add_(0.01)
    m2.load_state_dict({k: torch.from_numpy(v) for k, v in before.items()})
    m2.eval()
    m.eval()
    us = torch.arange(6)
    np.testing.assert_array_equal(m2._scores(us).cpu().numpy(), m._scores(us).cpu().numpy())


def test_large_catalogue_step_against_oracle():
    """I = 90 000 items, the default widths: one training step against the float64 oracle, relative to each tensor's
    update (SGD: the update IS lr * gradient)"""
    from daisyrec_amd.model import VAECF
    rng = np.random.default_rng(9)
    U, I, B, L = 64, 90000, 32, 300
    hid = np.zeros((U, L), dtype=np.int64)
    hval = np.zeros((U, L), dtype=np.float32)
    for u in range(U):
        n = int(rng.integers(20, L))
        hid[u, :n] = np.sort(rng.choice(I, size=n, replace=False))
        hval[u, :n] = 1.0
    torch.manual_seed(1)
    m = VAECF(vae_config(user_num=U, item_num=I, lr=1.0, optimizer="sgd", history_item_id=torch.from_numpy(hid),
                         history_item_value=torch.from_numpy(hval)))
    init = host_state(m)
    users = rng.choice(U, size=B, replace=False)
    R = m.get_user_rating_matrix(torch.from_numpy(users)).cpu().numpy()
    keep = (rng.random(int((R != 0).sum())) >= 0.5).astype(np.uint8)
    eps = rng.standard_normal((B, 64)).astype(np.float32)
    losses = replay(m, [(users, keep, eps)], "sgd", 0.5, 0.2, 100000)
    ol, op = VO.run_steps(init, [(R, keep, eps)], 128, "sgd", 1.0, 0.5, 0.2, 100000)
    assert abs(losses[0] - ol[0]) <= 1e-5 * abs(ol[0])
    got = host_state(m)
    for k, ref in op.items():
        upd, upd_o = got[k] - init[k], ref.numpy() - init[k]
        err = np.abs(upd - upd_o).max() / max(np.abs(upd_o).max(), 1e-30)
        assert err <= 1e-4, (k, err)


def test_torch_op_matches_the_model(kat):
    import daisyrec_amd.torch_ops  # noqa: F401
    m = kat_model(kat, "vae_adam")
    m.eval()
    W = m._params()
    csr, lens = m._csr()
    us = torch.tensor([0, 3, 5, 7])
    cands = torch.tensor([[1, 2, 3], [4, 5, 6], [0, 7, 9], [10, 11, 12]]).cuda()
    ref = m._scores(us, cands)
    got = torch.ops.daisyrec.vae_scores(W, csr[0], csr[1], csr[2], us.cuda(), cands, m.layers, m.lat_dim, m.item_num)
    torch.testing.assert_close(got, ref, rtol=0, atol=0)


def _fit_setup(ml, total, cap, B=128):
    """a loader over the training users in dataset order, the batches it yields, a fresh model"""
    from torch.utils.data import DataLoader, Dataset

    class Users(Dataset):                                  # what AEDataset holds: the training users
        def __init__(self, data):
            self.data = data

        def __len__(self):
            return len(self.data)

        def __getitem__(self, k):
            return self.data[k]
    users = np.nonzero(ml["ml/hist_len"])[0]
    loader = DataLoader(Users(users), batch_size=B, shuffle=False)
    batches = [users[k:k + B] for k in range(0, len(users), B)]
    return loader, batches, (lambda: ml_model(ml, total_anneal_steps=total, anneal_cap=cap, epochs=1))


def _replay_hash(m, epochs, seed_steps0=0, update0=0, optim=None):
    """what fit_epoch must compute, one step_grads + dense optimiser step at a time from Python: step k of the fit uses
    the device noise of seed (seed << 32) | k and anneal f32(min(cap, update / total)).  epochs: [[users of batch]]"""
    from daisyrec_amd import ops
    from daisyrec_amd import _native as N
    W = m._params()
    csr, lens = m._csr()
    B = max(len(b) for e in epochs for b in e)
    E = max(int(lens[torch.as_tensor(b)].sum()) for e in epochs for b in e)
    ctx = ops.VaeContext(B, E, m.item_num, m.layers, m.lat_dim)
    optim = optim if optim is not None else ops.DenseOptimizer("adam", m.lr)
    g = torch.zeros_like(W)
    seed_hi = (int(m.seed) & 0xFFFFFFFF) << 32
    step, update, sums = seed_steps0, update0, []
    for batches in epochs:
        acc = 0.0
        for users in batches:
            step += 1
            update += 1
            users = torch.as_tensor(users, dtype=torch.int64)
            ctx.step_grads(W, g, csr, users.cuda(), int(lens[users].sum()), train=True, dropout=m.dropout,
                           anneal=f32(VO.anneal_at(update, m.anneal_cap, m.total_anneal_steps)), seed=seed_hi | step)
            acc += float(ctx.stats[N.VST_LOSS])
            optim.next_step()
            optim.step(W, g)
        sums.append(acc)
    ctx.close()
    return sums, optim


def test_fit_epoch_equals_the_step_replay(ml):
    """VAECF.fit runs daisy_vae_fit_epoch: its parameters and epoch losses are the bits of step_grads + the dense Adam
    replayed step by step with the per-step seed and anneal (anneal still rising through the second epoch)"""
    loader, batches, make = _fit_setup(ml, total=0, cap=0.0)
    nb = len(batches)
    a = make()
    a.total_anneal_steps, a.anneal_cap, a.epochs = 2 * nb + 3, 0.9, 2
    a.fit(loader)
    b = make()
    b.total_anneal_steps, b.anneal_cap = 2 * nb + 3, 0.9
    sums, _ = _replay_hash(b, [batches, batches])
    assert a.epoch_losses == sums
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    assert a.update == 2 * nb and a._steps == 2 * nb


@pytest.mark.parametrize("opt,width", [pytest.param(o, w, id=o if w == 8 else f"{o}-width{w}") for w in (8, 6)
                                       for o in ("sgd", "adam", "adagrad", "rmsprop")])
def test_fit_epoch_equals_step_grads_plus_the_dense_optimiser(opt, width):
    """daisy_vae_fit_epoch against daisy_vae_step_grads + daisy_{sgd,adam,adagrad,rmsprop}_dense issued step by step:
    the flat parameters and the optimiser state bit for bit.  12 users x 40 items in batches of 5 (three steps, the last
    one of 2 users), hidden [8] (the float4 entry kernels) or [6] (the scalar ones: the library-issued epoch runs
    k_vae_enc0 / k_vae_w0grad too), latent 4, the anneal still rising; the optimiser starts at step 5 and the noise at
    step 9, so a loop that fed Adam the wrong counter would show in the bias correction."""
    from daisyrec_amd import ops
    from daisyrec_amd import _native as N
    from daisyrec_amd.model import VAECF
    rng = np.random.default_rng(3)
    U, I, Lh, B, t0, s0, u0 = 12, 40, 9, 5, 5, 9, 2
    hid = np.zeros((U, Lh), dtype=np.int64)
    hval = np.zeros((U, Lh), dtype=np.float32)
    for u in range(U):
        k = int(rng.integers(3, Lh + 1))
        hid[u, :k] = np.sort(rng.choice(np.arange(1, I), size=k, replace=False))
        hval[u, :k] = 1.0
    users = torch.as_tensor(rng.permutation(U), dtype=torch.int64)
    cap, total = 0.9, 8

    def run(native):
        torch.manual_seed(2)
        m = VAECF(vae_config(user_num=U, item_num=I, mlp_hidden_size=[width], latent_dim=4, dropout=0.0, lr=0.01, seed=7,
                             anneal_cap=cap, total_anneal_steps=total, history_item_id=torch.from_numpy(hid),
                             history_item_value=torch.from_numpy(hval)))
        W = m._params()
        init = W.cpu().numpy().copy()
        csr, lens = m._csr()
        entries = [int(x.sum()) for x in torch.split(lens[users], B)]
        g = torch.zeros_like(W)
        optim = ops.DenseOptimizer(opt, m.lr)
        optim.t = t0
        seed_hi = (int(m.seed) & 0xFFFFFFFF) << 32
        ctx = ops.VaeContext(B, max(entries), I, m.layers, m.lat_dim)
        try:
            if native:
                steps = ctx.fit_epoch(W, g, csr, users.cuda(), B, entries, optim, 0.0, cap, total, u0, seed_hi=seed_hi, step0=s0)
                loss = float(ctx.stats[N.VST_LOSS_SUM].cpu())
            else:
                steps, loss = 0, 0.0
                for k, us in enumerate(torch.split(users, B)):
                    steps += 1
                    ctx.step_grads(W, g, csr, us.cuda(), entries[k], train=True, dropout=0.0,
                                   anneal=f32(VO.anneal_at(u0 + steps, cap, total)), seed=seed_hi | (s0 + steps))
                    loss += float(ctx.stats[N.VST_LOSS])
                    optim.next_step()
                    optim.step(W, g)
        finally:
            ctx.close()
        return steps, optim.t, loss, W.cpu().numpy().copy(), [x.cpu().numpy().copy() for x in optim.state_for(W)], init

    a, b = run(True), run(False)
    assert a[0] == b[0] == 3 and a[1] == b[1] == t0 + 3
    assert a[2] == b[2] and np.isfinite(a[2]) and a[2] > 0
    assert np.array_equal(a[3].view(np.uint8), b[3].view(np.uint8)) and not np.array_equal(a[3], a[5])
    assert len(a[4]) == len(b[4]) == {"sgd": 0, "adam": 2, "adagrad": 1, "rmsprop": 1}[opt]
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a[4], b[4]))


def test_second_fit_carries_anneal_and_restarts_adam(ml):
    """two fits = one replay of both whose Adam restarts at the boundary (a fresh optimiser per fit) while the update
    counter and the noise keys carry on; a replay that keeps the first fit's Adam state gives other bits"""
    from daisyrec_amd import ops
    loader, batches, make = _fit_setup(ml, total=0, cap=0.0)
    nb = len(batches)
    total = 2 * nb                                        # anneal = update / total < cap through both fits
    a = make()
    a.total_anneal_steps, a.anneal_cap = total, 0.9
    a.fit(loader)
    a.fit(loader)
    assert a.update == 2 * nb
    b = make()
    b.total_anneal_steps, b.anneal_cap = total, 0.9
    s1, _ = _replay_hash(b, [batches])
    s2, _ = _replay_hash(b, [batches], seed_steps0=nb, update0=nb)       # a fresh Adam
    assert a.epoch_losses == s2
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    c = make()
    c.total_anneal_steps, c.anneal_cap = total, 0.9
    _, opt = _replay_hash(c, [batches])
    _replay_hash(c, [batches], seed_steps0=nb, update0=nb, optim=opt)    # Adam continued: must differ
    assert any(not torch.equal(v, c.state_dict()[k]) for k, v in a.state_dict().items())
    d = make()                                            # the anneal carried: restarting it from 0 must differ
    d.total_anneal_steps, d.anneal_cap = total, 0.9
    _replay_hash(d, [batches])
    s2d, _ = _replay_hash(d, [batches], seed_steps0=nb, update0=0, optim=ops.DenseOptimizer("adam", d.lr))
    assert s2d != s2


def test_calc_loss_is_the_first_steps_loss(ml):
    """VAECF.calc_loss in training mode: the loss of the step fit would take next (same noise key, same anneal), no
    parameter change, update counted like the reference"""
    loader, batches, make = _fit_setup(ml, total=0, cap=0.0)
    a = make()
    a.total_anneal_steps, a.anneal_cap = 7, 0.9
    before = host_state(a)
    a.train()
    loss = float(a.calc_loss(torch.as_tensor(batches[0])))
    assert a.update == 1
    after = host_state(a)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    b = make()
    b.total_anneal_steps, b.anneal_cap = 7, 0.9
    sums, _ = _replay_hash(b, [[batches[0]]])
    assert loss == sums[0]
    a.eval()                                              # eval mode: no dropout, z = mu - another number, finite
    l_eval = float(a.calc_loss(torch.as_tensor(batches[0])))
    assert np.isfinite(l_eval) and l_eval != loss and a.update == 2


def test_undercounted_entries_are_flagged_and_padded(ml):
    """n_entries below the batch's real count: the rows past it are flagged bad and left out, every entry the sort reads
    is the sentinel - the gradient equals that of the batch without those rows"""
    from daisyrec_amd import ops
    from daisyrec_amd import _native as N
    m = ml_model(ml)
    W = m._params()
    csr, lens = m._csr()
    users = torch.from_numpy(np.nonzero(ml["ml/hist_len"])[0][:64])
    L = lens[users]
    cut = int(L[:40].sum()) + int(L[40]) // 2            # row 40 straddles the count, rows 41.. lie past it
    ctx = ops.VaeContext(64, int(L.sum()), m.item_num, m.layers, m.lat_dim)
    g1, g2 = torch.zeros_like(W), torch.zeros_like(W)
    ctx.step_grads(W, g1, csr, users.cuda(), cut, train=False, anneal=0.1)
    assert float(ctx.stats[N.VST_BAD_ROWS]) == 24
    # the first 40 rows alone: the encoder-input gradient touches exactly the same item rows
    ctx.step_grads(W, g2, csr, users[:40].cuda(), int(L[:40].sum()), train=False, anneal=0.1)
    n0 = m.item_num * m.layers[0]
    touched1 = g1[:n0].view(m.item_num, -1).abs().sum(1) != 0
    touched2 = g2[:n0].view(m.item_num, -1).abs().sum(1) != 0
    assert bool(touched1.any()) and torch.equal(touched1, touched2)
    ctx.close()
