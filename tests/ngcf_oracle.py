"""Float64 restatement of NGCF (daisy/model/NGCFRecommender.py:19-209) for the tests: the forward written out from
the formulas, the gradients from torch autograd on the CPU, so they do not share the HIP backward's derivation.
A_hat comes from oracle.lightgcn_numpy.norm_adj_csr.  Dropout masks are explicit arguments (the device draws them
from a counter hash; tests read them back through ops.dropout_mask)."""
import numpy as np
import torch

from oracle import lightgcn_numpy as LG

LOSSES = ("BPR", "HL", "TL", "CL", "SL")


def adj(users, items, U, I):
    """A_hat as (indptr, col, val) (rows, then columns ascending: the device graph's entry order)."""
    return LG.norm_adj_csr(users, items, U, I)


def _sparse(graph, n, node_keep=None, node_p=0.0, dtype=torch.float64):
    indptr, col, val = graph
    rows = np.repeat(np.arange(n), np.diff(indptr))
    v = torch.as_tensor(np.asarray(val, np.float32)).to(dtype)
    if node_keep is not None:                           # SparseDropout (:19-36): kept entries scaled by 1 / (1 - p)
        k = torch.as_tensor(np.asarray(node_keep, bool))
        v = torch.where(k, v * (1.0 / (1.0 - node_p)), torch.zeros_like(v))
    idx = torch.as_tensor(np.stack([rows, np.asarray(col, np.int64)]))
    return torch.sparse_coo_tensor(idx, v, (n, n)).coalesce()


def layer(A, E, W1, b1, W2, b2, mess_keep=None, mess_p=0.0):
    """one BiGNN layer + LeakyReLU + message dropout + F.normalize (:52-60, :163-167); torch tensors"""
    X = torch.sparse.mm(A, E)
    Z = (E + X) @ W1.T + b1 + (X * E) @ W2.T + b2
    H = torch.where(Z > 0, Z, 0.2 * Z)
    if mess_keep is not None:
        H = H * torch.as_tensor(np.asarray(mess_keep, bool)).to(H.dtype) * (1.0 / (1.0 - mess_p))
    n = H.norm(dim=1, keepdim=True)
    return H / n.clamp_min(1e-12), X, n[:, 0]


def _t(x, dtype=torch.float64, grad=False):
    t = torch.as_tensor(np.asarray(x)).to(dtype).clone()
    t.requires_grad_(grad)
    return t


def forward(graph, params, widths, node_keep=None, node_p=0.0, mess_keeps=None, mess_p=0.0, grad=False):
    """out = [E0 | E1 | ... | EL] (:158-172).  params: dict of numpy arrays under the reference's state_dict names.
    Returns (out, torch params dict)."""
    tp = {k: _t(v, grad=grad) for k, v in params.items()}
    n = tp["embed_user.weight"].shape[0] + tp["embed_item.weight"].shape[0]
    A = _sparse(graph, n, node_keep, node_p)
    E = torch.cat([tp["embed_user.weight"], tp["embed_item.weight"]], 0)
    outs = [E]
    for k in range(len(widths) - 1):
        p = f"gnn_layers.{k}."
        E, _, _ = layer(A, E, tp[p + "linear.weight"], tp[p + "linear.bias"], tp[p + "interact_transform.weight"],
                        tp[p + "interact_transform.bias"], None if mess_keeps is None else mess_keeps[k], mess_p)
        outs.append(E)
    return torch.cat(outs, 1), tp


def criterion(loss_type, pos, neg_or_label, gamma=1e-10):
    lt = loss_type.upper()
    if lt == "BPR":
        return -(gamma + torch.sigmoid(pos - neg_or_label)).log().sum()
    if lt == "HL":
        return torch.clamp(1 - (pos - neg_or_label), min=0).sum()
    if lt == "TL":
        return (neg_or_label - pos).sigmoid().sum() + neg_or_label.pow(2).sigmoid().sum()
    if lt == "CL":
        return torch.nn.functional.binary_cross_entropy_with_logits(pos, neg_or_label, reduction="sum")
    if lt == "SL":
        return torch.nn.functional.mse_loss(pos, neg_or_label, reduction="sum")
    raise NotImplementedError(f"Invalid loss type: {loss_type}")


def loss_and_grads(graph, params, widths, u, i, j, loss_type, reg_1, reg_2, node_keep=None, node_p=0.0,
                   mess_keeps=None, mess_p=0.0):
    """calc_loss (:174-209) and the gradients of every parameter (numpy float64 dict)."""
    out, tp = forward(graph, params, widths, node_keep, node_p, mess_keeps, mess_p, grad=True)
    U = params["embed_user.weight"].shape[0]
    u, i, j = (torch.as_tensor(np.asarray(x, np.int64)) for x in (u, i, j))
    ue, pe = out[u], out[U + i]
    pos = (ue * pe).sum(1)
    ego_u, ego_i = tp["embed_user.weight"][u], tp["embed_item.weight"][i]
    if loss_type.upper() in ("CL", "SL"):
        loss = criterion(loss_type, pos, j.to(torch.float64))
        loss = loss + reg_1 * (ego_u.norm(p=1) + ego_i.norm(p=1))
        loss = loss + reg_2 * (ego_u.norm() + ego_i.norm())
    else:
        neg = (ue * out[U + j]).sum(1)
        ego_j = tp["embed_item.weight"][j]
        loss = criterion(loss_type, pos, neg)
        loss = loss + reg_1 * (ego_u.norm(p=1) + ego_i.norm(p=1) + ego_j.norm(p=1))
        loss = loss + reg_2 * (ego_u.norm() + ego_i.norm() + ego_j.norm())
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy().copy() for k, v in tp.items()}


def layer_grads(graph, E, W1, b1, W2, b2, dY, node_keep=None, node_p=0.0, mess_keep=None, mess_p=0.0):
    """One layer on its own: Y, X, norm and the gradients of <Y, dY> wrt E, W1, b1, W2, b2 (float64 numpy).
    dE includes the path through X = A_hat E."""
    n = E.shape[0]
    A = _sparse(graph, n, node_keep, node_p)
    Et, W1t, b1t, W2t, b2t = (_t(x, grad=True) for x in (E, W1, b1, W2, b2))
    Y, X, nrm = layer(A, Et, W1t, b1t, W2t, b2t, mess_keep, mess_p)
    (Y * _t(dY)).sum().backward()
    return (Y.detach().numpy(), X.detach().numpy(), nrm.detach().numpy(),
            {"E": Et.grad.numpy(), "W1": W1t.grad.numpy(), "b1": b1t.grad.numpy(), "W2": W2t.grad.numpy(),
             "b2": b2t.grad.numpy()})


def dense_layer_grads(E, X, W1, b1, W2, b2, dY, mess_keep=None, mess_p=0.0):
    """The dense part of one layer with X given (no graph): Y, norm and the gradients wrt E (through S and T only),
    X, W1, b1, W2, b2 - what daisy_ngcf_layer_backward returns as dE, dX and the weight gradients."""
    Et, Xt, W1t, b1t, W2t, b2t = (_t(x, grad=True) for x in (E, X, W1, b1, W2, b2))
    Z = (Et + Xt) @ W1t.T + b1t + (Xt * Et) @ W2t.T + b2t
    H = torch.where(Z > 0, Z, 0.2 * Z)
    if mess_keep is not None:
        H = H * torch.as_tensor(np.asarray(mess_keep, bool)).to(H.dtype) * (1.0 / (1.0 - mess_p))
    nrm = H.norm(dim=1, keepdim=True)
    Y = H / nrm.clamp_min(1e-12)
    (Y * _t(dY)).sum().backward()
    return (Y.detach().numpy(), nrm[:, 0].detach().numpy(),
            {"E": Et.grad.numpy(), "X": Xt.grad.numpy(), "W1": W1t.grad.numpy(), "b1": b1t.grad.numpy(),
             "W2": W2t.grad.numpy(), "b2": b2t.grad.numpy()})


def adam_step(params, grads, state, lr, t, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam (defaults, float64) on every parameter; state: dict name -> (m, v), created on first use."""
    out = {}
    for k, p in params.items():
        g = grads[k]
        m, v = state.get(k, (np.zeros_like(p, np.float64), np.zeros_like(p, np.float64)))
        m = betas[0] * m + (1 - betas[0]) * g
        v = betas[1] * v + (1 - betas[1]) * g * g
        state[k] = (m, v)
        denom = np.sqrt(v) / np.sqrt(1 - betas[1] ** t) + eps
        out[k] = p - lr / (1 - betas[0] ** t) * m / denom
    return out


def sgd_step(params, grads, lr):
    return {k: p - lr * grads[k] for k, p in params.items()}


def run_steps(graph, params, widths, batches, loss_type, reg_1, reg_2, optimizer, lr):
    """The reference's training loop over explicit batches (no dropout): losses and final parameters."""
    p = {k: np.asarray(v, np.float64) for k, v in params.items()}
    state, losses = {}, []
    for t, (u, i, j) in enumerate(batches, 1):
        loss, g = loss_and_grads(graph, p, widths, u, i, j, loss_type, reg_1, reg_2)
        losses.append(loss)
        p = adam_step(p, g, state, lr, t) if optimizer == "adam" else sgd_step(p, g, lr)
    return np.array(losses), p
