"""Float64 restatement of NFM (daisy/model/NFMRecommender.py:110-151) for the tests: the forward written out from the
formulas (BatchNorm in training mode with its own batch statistics per forward call), the gradients from torch
autograd on the CPU, the optimiser step from torch.optim.  Dropout masks are explicit arguments (the device draws them
from a counter hash; tests read them back through ops.dropout_mask)."""
import numpy as np
import torch

LOSSES = ("BPR", "HL", "TL", "CL", "SL")
EPS, MOMENTUM = 1e-5, 0.1


def act_fn(name):
    return {"relu": torch.relu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}.get(name, lambda x: x)


def stage_names(state, L, bn):
    """state_dict prefixes of the Linear and BatchNorm modules (deep_layers indices shift without an activation)."""
    keys = list(state)
    lin = sorted({k.rsplit(".", 1)[0] for k in keys if k.startswith("deep_layers.") and state[k].ndim == 2},
                 key=lambda s: int(s.split(".")[1]))
    bns = []
    if bn:
        bns = ["FM_layers.0"] + sorted({k.rsplit(".", 1)[0] for k in keys if k.startswith("deep_layers.")
                                        and k.endswith("running_mean")}, key=lambda s: int(s.split(".")[1]))
    assert len(lin) == L and (not bn or len(bns) == L + 1)
    return lin, bns


def forward(t, bufs, u, i, L, bn, act, train=True, masks=None, p=0.0):
    """pred [n] of one forward call; t: name -> float64 tensor (parameters), bufs: name -> tensor (running stats,
    updated in place in training mode).  masks: stage -> bool [n, d] keep mask (or None)."""
    lin, bns = stage_names({**t, **bufs}, L, bn)
    f = act_fn(act)
    x = t["embed_user.weight"][u] * t["embed_item.weight"][i]
    for s in range(L + 1):
        if s > 0:
            x = h @ t[f"{lin[s - 1]}.weight"].T + t[f"{lin[s - 1]}.bias"]
        if bn:
            n = bns[s]
            if train:
                m, v = x.mean(0), x.var(0, unbiased=False)
                with torch.no_grad():
                    cnt = x.shape[0]
                    bufs[f"{n}.running_mean"].mul_(1 - MOMENTUM).add_(MOMENTUM * m.detach())
                    bufs[f"{n}.running_var"].mul_(1 - MOMENTUM).add_(MOMENTUM * v.detach() * cnt / (cnt - 1))
                    bufs[f"{n}.num_batches_tracked"] += 1
            else:
                m, v = bufs[f"{n}.running_mean"], bufs[f"{n}.running_var"]
            y = (x - m) / torch.sqrt(v + EPS) * t[f"{n}.weight"] + t[f"{n}.bias"]
        else:
            y = x
        a = f(y) if s > 0 else y
        if masks is not None and masks.get(s) is not None:
            a = a * torch.as_tensor(np.asarray(masks[s], bool)).to(a.dtype) * (1.0 / (1.0 - p))
        h = a
    bias = t["u_bias.weight"][u] + t["i_bias.weight"][i] + t["bias_"]
    return ((h + bias) @ t["prediction.weight"].T).view(-1)


def criterion(loss_type, pos, neg_or_label):
    if loss_type == "BPR":
        return -(1e-10 + torch.sigmoid(pos - neg_or_label)).log().sum()
    if loss_type == "HL":
        return torch.clamp(1 - (pos - neg_or_label), min=0).sum()
    if loss_type == "TL":
        return torch.sigmoid(neg_or_label - pos).sum() + torch.sigmoid(neg_or_label ** 2).sum()
    if loss_type == "CL":
        return torch.nn.functional.binary_cross_entropy_with_logits(pos, neg_or_label, reduction="sum")
    return torch.nn.functional.mse_loss(pos, neg_or_label, reduction="sum")


def calc_loss(t, bufs, u, i, j, L, bn, act, loss_type, reg_1, reg_2, masks=(None, None), p=0.0):
    """NFM.calc_loss (:125-151): the pairwise losses forward twice (positives first)."""
    u, i, j = (torch.as_tensor(np.asarray(x, np.int64)) for x in (u, i, j))
    P, Q = t["embed_user.weight"], t["embed_item.weight"]
    pos = forward(t, bufs, u, i, L, bn, act, True, masks[0], p)
    if loss_type in ("CL", "SL"):
        loss = criterion(loss_type, pos, j.to(pos.dtype))
        loss = loss + reg_1 * Q[i].norm(p=1) + reg_2 * Q[i].norm()
    else:
        neg = forward(t, bufs, u, j, L, bn, act, True, masks[1], p)
        loss = criterion(loss_type, pos, neg)
        loss = loss + reg_1 * (Q[i].norm(p=1) + Q[j].norm(p=1)) + reg_2 * (Q[i].norm() + Q[j].norm())
    return loss + reg_1 * P[u].norm(p=1) + reg_2 * P[u].norm()


def zero_grad_params(state, L, bn):
    """Parameters whose exact gradient is 0 with batch_norm: a Linear bias, and the BatchNorm shift of every stage
    before the last, feed a BatchNorm whose batch mean removes them.  Their computed gradients are rounding noise,
    which Adam scales up to steps of about lr: no two implementations agree on them - nor on the running means of
    the stages after the first, which they shift (the losses and every other parameter do not see them)."""
    if not bn:
        return set()
    lin, bns = stage_names(state, L, bn)
    return ({f"{n}.bias" for n in lin} | {f"{n}.bias" for n in bns[:-1]}
            | {f"{n}.running_mean" for n in bns[1:]})


def split_state(state):
    """state_dict -> (float64 parameters requiring grad, buffers)"""
    params, bufs = {}, {}
    for k, v in state.items():
        v = torch.as_tensor(np.array(v))
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            bufs[k] = v.to(torch.float64) if v.is_floating_point() else v.clone()
        else:
            params[k] = v.to(torch.float64).requires_grad_(True)
    return params, bufs


def run_steps(state, steps, L, bn, act, loss_type, optimizer, lr, reg_1, reg_2, masks=None, p=0.0):
    """steps: list of (u, i, j).  Returns (losses, params, bufs) after the optimiser steps (torch.optim, float64)."""
    params, bufs = split_state(state)
    opts = {"sgd": torch.optim.SGD, "adam": torch.optim.Adam,
            "adagrad": lambda ps, lr: torch.optim.Adagrad(ps, lr=lr, eps=1e-10),
            "rmsprop": lambda ps, lr: torch.optim.RMSprop(ps, lr=lr, alpha=0.99, eps=1e-8)}
    opt = opts[optimizer](list(params.values()), lr=lr)
    losses = []
    for k, (u, i, j) in enumerate(steps):
        opt.zero_grad()
        loss = calc_loss(params, bufs, u, i, j, L, bn, act, loss_type, reg_1, reg_2,
                         masks[k] if masks is not None else (None, None), p)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, {k: v.detach() for k, v in params.items()}, bufs
