"""Float64 autograd oracle of VAECF's training step (daisy/model/VAECFRecommender.py:79-110) with EXPLICIT noise: the
input dropout's keep bits where R != 0 (row-major) and the reparameterisation's eps.  Parameters are dicts in the
reference's state_dict layout; the optimisers are torch's own, in float64."""
import numpy as np
import torch
import torch.nn.functional as F

OPTIMIZERS = {"adam": torch.optim.Adam, "sgd": torch.optim.SGD, "adagrad": torch.optim.Adagrad,
              "rmsprop": torch.optim.RMSprop}


def linear_names(state, prefix):
    """the Linear layers of an nn.Sequential in order: [(weight key, bias key)]"""
    idx = sorted({int(k.split(".")[1]) for k in state if k.startswith(prefix + ".")})
    return [(f"{prefix}.{i}.weight", f"{prefix}.{i}.bias") for i in idx]


def mlp(x, P, layers):
    for k, (w, b) in enumerate(layers):
        x = F.linear(x, P[w], P[b])
        if k != len(layers) - 1:
            x = torch.tanh(x)
    return x


def forward(P, R, lat, keep=None, eps=None, p=0.5, train=True, dtype=torch.float64):
    """(logits, mu, logvar) in `dtype` (the parameters' own); R: dense [B, I]"""
    R = R.to(dtype)
    h = F.normalize(R)
    if train and p > 0:
        mask = torch.zeros_like(R)
        mask[R != 0] = torch.as_tensor(keep, dtype=R.dtype)
        h = h * mask / (1.0 - p)
    h = mlp(h, P, linear_names(P, "encoder"))
    mu, logvar = h[:, :lat // 2], h[:, (lat + 1) // 2:]
    z = torch.as_tensor(eps, dtype=R.dtype) * torch.exp(0.5 * logvar) + mu if train else mu
    return mlp(z, P, linear_names(P, "decoder")), mu, logvar


def loss_of(P, R, lat, keep, eps, p, anneal, train=True, dtype=torch.float64):
    R = R.to(dtype)
    z, mu, logvar = forward(P, R, lat, keep, eps, p, train, dtype)
    kl = -0.5 * torch.mean(torch.sum(1 + logvar - mu.pow(2) - logvar.exp(), dim=1)) * anneal
    ce = -(F.log_softmax(z, 1) * R).sum(1).mean()
    return ce + kl


def anneal_at(update, cap, total):
    return min(cap, 1.0 * update / total) if total > 0 else cap


def run_steps(state, steps, lat, optimizer, lr, p, cap, total, update0=0):
    """steps: [(R [B, I], keep, eps)].  Returns (losses, final params as float64 tensors, gradients of the last step)."""
    P = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in state.items()}
    opt = OPTIMIZERS[optimizer](list(P.values()), lr=lr)
    losses, update = [], update0
    for R, keep, eps in steps:
        update += 1
        opt.zero_grad()
        loss = loss_of(P, torch.as_tensor(np.asarray(R), dtype=torch.float64), lat, keep, eps, p,
                       anneal_at(update, cap, total))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return np.array(losses), {k: v.detach() for k, v in P.items()}


def grads_of(state, R, lat, keep, eps, p, anneal, train=True, dtype=torch.float64):
    """(loss, gradient of every parameter) of one step in `dtype`: float64 is the oracle; with torch.float32 the same code
    is a plain fp32 restatement of the reference's arithmetic"""
    P = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in state.items()}
    loss = loss_of(P, torch.tensor(np.asarray(R), dtype=dtype), lat, keep, eps, p, anneal, train, dtype)
    loss.backward()
    return float(loss.detach()), {k: v.grad.detach().numpy() for k, v in P.items()}
