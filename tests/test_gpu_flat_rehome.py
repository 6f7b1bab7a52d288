"""A model whose parameters were re-homed between two fits (`model.cpu(); model.cuda()`) trains like one that was not.

Every parameter is on the device after the round trip, but none is a view of the model's flat buffer any more: a fit that
tested only "is it on the device?" handed the kernels the new tensors and the dense optimiser the old buffer, and trained
nothing.  Two models from one seed, two fits each, the round trip on one of them in between: bit-equal state dicts and
losses.  VAECF, which always compared addresses, is the control."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import mf_config

pytestmark = pytest.mark.gpu

U, I, D, N_ROWS, B = 40, 30, 8, 64, 32          # two optimiser steps per epoch


def _rows():
    rng = np.random.default_rng(3)
    u = (np.arange(N_ROWS) % U).astype(np.int32)            # every user has a history (VAECF trains all 40)
    return np.stack([u, rng.integers(0, I, N_ROWS).astype(np.int32), rng.integers(0, I, N_ROWS).astype(np.int32)], 1)


def _build(name, rows):
    from daisyrec_amd import model as M
    base = dict(user_num=U, item_num=I, factors=D, epochs=1, lr=0.05, reg_1=0.0, reg_2=0.0, optimizer="sgd", batch_size=B,
                seed=5)
    graph = sp.coo_matrix((np.ones(N_ROWS, np.float32), (rows[:, 0], rows[:, 1])), shape=(U, I))
    if name == "NeuMF":
        cfg = mf_config(algo_name="neumf", num_layers=2, dropout=0.0, model_name="NeuMF", GMF_model=None, MLP_model=None, **base)
    elif name == "NFM":
        cfg = mf_config(algo_name="nfm", num_layers=2, dropout=0.0, batch_norm=False, act_function="relu", **base)
    elif name == "NGCF":
        cfg = mf_config(algo_name="ngcf", hidden_size_list=[8, 8], node_dropout=0.0, mess_dropout=0.0, inter_matrix=graph, **base)
    elif name == "LightGCN":
        cfg = mf_config(algo_name="lightgcn", num_layers=2, inter_matrix=graph, **base)
    else:
        hist = [sorted(set(rows[rows[:, 0] == u, 1].tolist())) for u in range(U)]
        width = max(len(h) for h in hist)
        hid = torch.tensor([h + [0] * (width - len(h)) for h in hist], dtype=torch.int64)
        hval = torch.tensor([[1.0] * len(h) + [0.0] * (width - len(h)) for h in hist])
        cfg = mf_config(algo_name="multi-vae", mlp_hidden_size=[D], latent_dim=D, dropout=0.0, total_anneal_steps=100,
                        anneal_cap=0.2, history_item_id=hid, history_item_value=hval, **base)
    torch.manual_seed(11)
    return getattr(M, name)(cfg)


def _loader(name, rows, seed):
    from torch.utils.data import DataLoader
    from daisyrec_amd.utils.dataset import BasicDataset
    g = torch.Generator()
    g.manual_seed(seed)
    data = BasicDataset(np.arange(U, dtype=np.int64) if name == "VAECF" else rows)
    return DataLoader(data, batch_size=B, shuffle=True, generator=g, num_workers=0)


@pytest.mark.parametrize("name", ["NeuMF", "NFM", "NGCF", "LightGCN", "VAECF"])
def test_fit_after_a_device_round_trip_equals_the_fit_without_it(name):
    rows = _rows()
    a, b = _build(name, rows), _build(name, rows)
    for m in (a, b):
        m.fit(_loader(name, rows, 21))
    first = {k: v.detach().cpu().clone() for k, v in b.state_dict().items()}
    a.cpu()
    a.cuda()
    for m in (a, b):
        m.fit(_loader(name, rows, 22))
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sb:
        assert torch.equal(sa[k].cpu(), sb[k].cpu()), k
    assert a.epoch_losses == b.epoch_losses and len(b.epoch_losses) == 1 and np.isfinite(b.epoch_losses[0])
    assert any(not torch.equal(first[k], sb[k].cpu()) for k in sb)         # (the second fit did train)
