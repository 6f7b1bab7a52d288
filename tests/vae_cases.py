"""Seeded synthetic Multi-VAE steps at the shapes where csrc/vae.hip takes another path than the reference's KATs and the
ml-100k replay do (numpy + torch on the CPU only; nothing of the package is imported): scalar first-layer widths, more
than 1 024 columns, no hidden layer, more than 256 rows, item runs and history rows of 256 / 257 / 512 / 513 entries,
saturated logits, ratings other than 1.  Every case is a function of a fixed seed; `case(name)` and `oracle(name)` are
computed once per process and their arrays are read-only.

Item 0 stays out of every history, so the `(item 0, value 0)` padding of the history arrays cannot change a case: the
rating rows the model derives from `hist_id` / `hist_val` are `R` itself (tests/test_oracle_vae.py asserts it)."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import vae_oracle as VO

P_DROP, ANNEAL = 0.5, 0.2

#        name              B    I    hidden  lat
SHAPES = {
    "scalar_6":          (7,   40,  [6],    4),
    "scalar_deep_odd":   (7,   40,  [3, 5], 7),
    "scalar_1":          (5,   12,  [1],    2),
    "nohidden_scalar":   (9,   40,  [],     6),
    "nohidden_v4":       (9,   40,  [],     8),
    "wide_scalar":       (3,   12,  [1027], 4),
    "wide_v4":           (3,   12,  [1028], 4),
    # 300 rows with a history + 2 empty ones: "item 5 in all 300 rows" and "two empty rows" need 302 rows
    "runs_scalar":       (302, 37,  [6],    4),
    "runs_v4":           (302, 37,  [8],    4),
    "runs_ratings":      (302, 37,  [6],    5),
    "rows_scalar":       (6,   600, [6],    4),
    "rows_v4":           (6,   600, [8],    4),
    "hot_softmax":       (7,   700, [8],    4),
}
NAMES = list(SHAPES)
SEEDS = {name: 4100 + k for k, name in enumerate(NAMES)}

RUNS_EMPTY_ROWS = (3, 301)                     # the last one takes k_vae_prep's `b == B - 1` padding branch with len == 0
RUNS_ITEMS = {5: 300, 6: 256, 7: 257, 36: 256}  # item -> the rows it is in (36: the largest id, the last sorted run)
ROWS_LENS = (256, 257, 512, 513, 3, 0)
HOT_EMPTY_ROW = 2
HOT_BIAS = {5: 100.0, 261: -100.0, 517: 95.0,  # softmax thread 5 meets its maximum first and never rescales
            9: -100.0, 265: 0.0, 521: 100.0}   # softmax thread 9 rescales at every element


def init_state(rng, I, hidden, lat):
    """a state dict in the reference's layout (nn.Sequential indices: Linear, Tanh, Linear, ...): weights N(0, xavier),
    biases N(0, 0.1) so that a bias read at the wrong column shows"""
    enc = [I] + list(hidden) + [lat]
    dec = [lat // 2] + list(hidden)[::-1] + [I]
    state = {}
    for prefix, dims in (("encoder", enc), ("decoder", dec)):
        for k, (din, dout) in enumerate(zip(dims[:-1], dims[1:])):
            state[f"{prefix}.{2 * k}.weight"] = (rng.standard_normal((dout, din)) * np.sqrt(2.0 / (din + dout))).astype(np.float32)
            state[f"{prefix}.{2 * k}.bias"] = (rng.standard_normal(dout) * 0.1).astype(np.float32)
    return state


def bernoulli_rows(rng, B, I, q=0.3):
    R = (rng.random((B, I)) < q).astype(np.float64)
    R[:, 0] = 0.0
    return R


def runs_rows(rng, B, I, ratings):
    R = bernoulli_rows(rng, B, I)
    full = np.array([b for b in range(B) if b not in RUNS_EMPTY_ROWS])       # the 300 rows with a history, in batch order
    for item, n in RUNS_ITEMS.items():
        R[:, item] = 0.0
        rows = full[:n] if item != 36 else np.sort(rng.choice(full, size=n, replace=False))
        R[rows, item] = 1.0
    R[list(RUNS_EMPTY_ROWS)] = 0.0
    if ratings:
        R = R * rng.integers(1, 6, size=R.shape)
    return R


def rows_rows(rng, B, I):
    R = np.zeros((B, I))
    for b, n in enumerate(ROWS_LENS):
        R[b, rng.choice(np.arange(1, I), size=n, replace=False)] = 1.0
    return R


def hot_rows(rng, B, I):
    R = np.zeros((B, I))
    for b in range(B):
        if b != HOT_EMPTY_ROW:
            R[b, rng.choice(np.arange(1, I), size=int(rng.integers(5, 30)), replace=False)] = 1.0
    return R


def histories(R):
    """the padded [B, L] history arrays of R's rows (items ascending, then item 0 / value 0)"""
    B = R.shape[0]
    L = max(1, int((R != 0).sum(1).max()))
    hid = np.zeros((B, L), dtype=np.int64)
    hval = np.zeros((B, L), dtype=np.float32)
    for b in range(B):
        cols = np.nonzero(R[b])[0]
        hid[b, :cols.size] = cols
        hval[b, :cols.size] = R[b, cols]
    return hid, hval


def _freeze(x):
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def case(name):
    B, I, hidden, lat = SHAPES[name]
    rng = np.random.default_rng(SEEDS[name])
    if name.startswith("runs_"):
        R = runs_rows(rng, B, I, ratings=(name == "runs_ratings"))
    elif name.startswith("rows_"):
        R = rows_rows(rng, B, I)
    elif name == "hot_softmax":
        R = hot_rows(rng, B, I)
    else:
        R = bernoulli_rows(rng, B, I)
    state = init_state(rng, I, hidden, lat)
    if name == "hot_softmax":
        bias = rng.choice(np.array([-100.0, 0.0], dtype=np.float32), size=I)
        for item, v in HOT_BIAS.items():
            bias[item] = v
        state[f"decoder.{2 * len(hidden)}.bias"] = bias
    keep = (rng.random(int((R != 0).sum())) >= P_DROP).astype(np.uint8)      # row-major over R's non-zeros
    eps = rng.standard_normal((B, lat // 2)).astype(np.float32)
    hid, hval = histories(R)
    return SimpleNamespace(name=name, B=B, I=I, hidden=list(hidden), lat=lat, R=_freeze(R),
                           state={k: _freeze(v) for k, v in state.items()}, keep=_freeze(keep), eps=_freeze(eps),
                           p=P_DROP, anneal=ANNEAL, hist_id=_freeze(hid), hist_val=_freeze(hval))


def anneal_f32(c):
    """the anneal as the C ABI receives it (a float)"""
    return float(np.float32(c.anneal))


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(loss, {name: gradient}) of the case's training step from the float64 oracle"""
    c = case(name)
    loss, g = VO.grads_of(c.state, c.R, c.lat, c.keep.copy(), c.eps.copy(), c.p, anneal_f32(c))
    return loss, {k: _freeze(v) for k, v in g.items()}


@functools.lru_cache(maxsize=None)
def restated_f32(name):
    """the same step from the same code in torch.float32: the reference's own arithmetic"""
    c = case(name)
    loss, g = VO.grads_of(c.state, c.R, c.lat, c.keep.copy(), c.eps.copy(), c.p, anneal_f32(c), dtype=torch.float32)
    return loss, {k: _freeze(v) for k, v in g.items()}


def errors(loss, grads, name):
    """(relative loss error, {tensor: max |error| over the oracle tensor's largest element}) against the oracle"""
    ol, og = oracle(name)
    per = {k: float(np.abs(np.asarray(grads[k], np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))
           for k, ref in og.items()}
    return abs(loss - ol) / abs(ol), per


@functools.lru_cache(maxsize=None)
def eval_scores(name):
    """the eval-mode scores [B, I] (no dropout, z = mu) from the float64 oracle"""
    c = case(name)
    P = {k: torch.tensor(v, dtype=torch.float64) for k, v in c.state.items()}
    with torch.no_grad():
        z, _, _ = VO.forward(P, torch.tensor(c.R), c.lat, train=False)
    return _freeze(z.numpy())


@functools.lru_cache(maxsize=None)
def train_logits(name):
    """the training step's logits [B, I] from the float64 oracle"""
    c = case(name)
    P = {k: torch.tensor(v, dtype=torch.float64) for k, v in c.state.items()}
    with torch.no_grad():
        z, _, _ = VO.forward(P, torch.tensor(c.R), c.lat, c.keep.copy(), c.eps.copy(), c.p, train=True)
    return _freeze(z.numpy())
