"""Segment layouts of the MF step and an exact integer reference of it (tests/test_host_segment_layouts.py checks this
module, tests/test_gpu_segment_layouts.py runs it against every segmented-sum path of the library).

Layouts.  The MF step sums a batch's contributions per user and per item over entries sorted by row: the entries of one
row are a SEGMENT, a lane group takes a RUN of consecutive entries, a workgroup a CHUNK of runs.  What goes wrong in such
code is an alignment - a segment that starts on a chunk's first entry and fills it, one that ends one entry into the next
unit, one that ends on a unit's last entry - so `layouts(n)` states the alignments instead of drawing ids at random.
Every run and chunk of the library is a power of two (lanes per row x run length; workgroup / lanes per row), read off
the configurations for every row shape of dispatch_d:

    RunCfg          (segsum.hip, k_item_grad_chunked)    runs 2 .. 16, chunks 16 .. 256 entries   (kSegsumRowsRun: 32, 64)
    UserRunCfg      (bpr_train.hip, k_user_chunked)      runs 4 / 8,   chunks 32 .. 256 samples
    StagedUserCfg   (bpr_staged.h, 64 / 128 threads)     runs 2 / 4,   chunks  8 .. 64 samples
    StagedItemCfg   (dense, 128 and 256 threads)         runs 4 .. 16, chunks 16 .. 256 entries
    StagedItemCfg   (sparse, 128 and 256 threads)        runs 2 / 4,   chunks  8 .. 128 entries
    bpr_small.hip   (one workgroup per epoch)            batches up to kSmallBatchMax = 256 samples

The largest chunk anywhere is 256 entries, none is not a power of two, so the periods 1, 2, 4 .. 2048 cover every run and
chunk size (and up to eight chunks of the largest) without mirroring dispatch_d here.  A block of the two-level edge
chains is kEdgeBlock = 32 chunks, at most 8192 entries: the long-chain layouts (`long`) cross several of them.

Exactness.  With small-integer tables, reg_1 = reg_2 = 0, a power-of-two learning rate and the hinge loss (coefficients
in {-1, 0, +1}) or the squared loss (coefficients 2 (score - label)), every score, coefficient, gradient, updated row
and the loss is a dyadic rational.  `assert_exact_domain` checks that for every output row the sum of the ABSOLUTE
values of all its terms, in units of the learning rate, stays below 2^24: then every partial sum in any order - runs,
slots, edge chains, atomics - is exactly representable in fp32, and a kernel that sums every entry exactly once returns
the bits of `exact_step`.  No tolerance is involved.
"""
import numpy as np
import torch

PERIODS = tuple(1 << k for k in range(12))        # 1 .. 2048
LARGEST_CHUNK = 256                               # entries; see the table above
EXACT_CAP = 1 << 24
HL, SL = 1, 4                                     # DAISY_LOSS_HL / DAISY_LOSS_SL
LR = {HL: 2.0 ** -3, SL: 2.0 ** -10}
TABLE_RANGE = {HL: (-2, 2), SL: (-1, 1)}


# ----------------------------------------------------------------------------------------------------------------------
# layouts
# ----------------------------------------------------------------------------------------------------------------------
def period(n, p, lead):
    """one segment of `lead` entries (if any), then segments of p, then what is left of n as one last segment"""
    if lead < 0 or lead >= n or p < 1:
        return None
    out = [lead] if lead else []
    rest = n - lead
    out += [p] * (rest // p)
    if rest % p:
        out.append(rest % p)
    return out


def comb(n, a, b):
    """alternating segments of a and b entries, the rest of n as one last segment"""
    if a < 1 or b < 1:
        return None
    out, left, k = [], n, 0
    while left > 0:
        x = min(a if k % 2 == 0 else b, left)
        out.append(x)
        left -= x
        k += 1
    return out


def long(n, k):
    """one segment of n - 2k entries between k singletons on either side"""
    if n - 2 * k < 1:
        return None
    return [1] * k + [n - 2 * k] + [1] * k


def layouts(n, max_p=PERIODS[-1]):
    """(name, [segment lengths]) pairs, every list positive and summing to n; lists that repeat an earlier one are left out
    (at small n most periods collapse into `one`)"""
    seen = set()
    cands = [("one", [n]), ("ones", [1] * n)]
    cands += [(f"long({k})", long(n, k)) for k in (0, 1, 3)]
    for p in PERIODS:
        if p > max_p:
            break
        for lead in (0, 1, p - 1):
            cands.append((f"period({p},{lead})", period(n, p, lead)))
        cands.append((f"comb(1,{p - 1})", comb(n, 1, p - 1)))
        cands.append((f"comb(1,{p})", comb(n, 1, p)))
    for name, lens in cands:
        if lens is None or tuple(lens) in seen:
            continue
        seen.add(tuple(lens))
        yield name, list(lens)


def named(n, name):
    """the layout `name` of layouts(n) built directly (it may repeat another one)"""
    if name == "one":
        return [n]
    if name == "ones":
        return [1] * n
    kind, args = name.rstrip(")").split("(")
    args = [int(x) for x in args.split(",")]
    lens = {"period": period, "comb": comb, "long": long}[kind](n, *args)
    assert lens is not None, (n, name)
    return lens


def row_ids(n_segments):
    """increasing ids with gaps: 0, 1, 3, 4, 6, 7 ... - every third row of the table stays untouched"""
    k = np.arange(n_segments, dtype=np.int64)
    return k + k // 2


def rows_needed(n_segments):
    """a table size that exceeds the largest id of row_ids and leaves an untouched row behind it"""
    return int(n_segments + (n_segments - 1) // 2 + 2)


def batch(layout_u, layout_i, rng, pointwise=False):
    """(u, i, j, user_num, item_num): int32 arrays of B = sum(layout_u) samples whose user multiplicities are layout_u and
    whose item multiplicities are layout_i.  Pair-wise: layout_i sums to 2 B, the permuted item entries are dealt to i
    (first half) and j (second half); samples that got i == j exchange their j among themselves where the layout has
    more than one item.  Point-wise: layout_i sums to B and j holds labels in {0, 1}."""
    B = int(np.sum(layout_u))
    u = np.repeat(row_ids(len(layout_u)), layout_u)[rng.permutation(B)]
    items = np.repeat(row_ids(len(layout_i)), layout_i)
    if pointwise:
        assert len(items) == B, (len(items), B)
        i = items[rng.permutation(B)]
        j = rng.integers(0, 2, B)
    else:
        assert len(items) == 2 * B, (len(items), B)
        items = items[rng.permutation(2 * B)]
        i, j = items[:B].copy(), items[B:].copy()
        same = np.flatnonzero(i == j)
        if len(same) > 1 and len(layout_i) > 1:
            order = same[np.argsort(j[same], kind="stable")]
            shift = int(np.bincount(j[order]).max())        # past the longest run of equal items
            j[order] = np.roll(j[order], shift)
    return (u.astype(np.int32), i.astype(np.int32), j.astype(np.int32), rows_needed(len(layout_u)),
            rows_needed(len(layout_i)))


def int_tables(rng, user_num, item_num, d, loss):
    lo, hi = TABLE_RANGE[loss]
    return (rng.integers(lo, hi + 1, (user_num, d)).astype(np.float32),
            rng.integers(lo, hi + 1, (item_num, d)).astype(np.float32))


# ----------------------------------------------------------------------------------------------------------------------
# the exact step
# ----------------------------------------------------------------------------------------------------------------------
def _int_tensor(x, what, device):
    """an integer-valued array or tensor as int64 on `device` (an int64 tensor is taken as it is)"""
    t = torch.as_tensor(x, device=device) if not isinstance(x, torch.Tensor) else x.to(device)
    if t.dtype == torch.int64:
        return t
    r = t.to(torch.float64).round().to(torch.int64)
    assert bool((r.to(torch.float64) == t.to(torch.float64)).all()), f"{what}: not integer-valued"
    return r


def _rowmax(W):
    return W.abs().amax(1) if W.shape[1] else torch.zeros(W.shape[0], dtype=torch.int64, device=W.device)


def _segment_sum(inv, n_rows, vals):
    """sum of the rows of vals under each segment number (int64: the order of the additions does not matter)"""
    out = torch.zeros((n_rows,) + tuple(vals.shape[1:]), dtype=torch.int64, device=vals.device)
    return out.index_add_(0, inv, vals)


class ExactStep:
    """One SGD step with reg 0 in int64 (torch tensors on the device the step was computed on): `loss` (int); the touched
    rows of either table (`urows`, `irows`, ascending) and their gradients gP / gQ (the data term: there is no other);
    `g_i_bias`, the per-item sum of the coefficients (FM).  What bounds the sums, whatever their order: aP / aQ (per
    touched row: the sum over its entries of |coefficient| x the largest |element| of the row that entry adds - at
    least the sum of |term| of every element), a_i_bias, `abs_score` (per sample sum_k |p||q| + |biases|, the largest)
    and `abs_loss` (the sum of the |terms| of the loss)."""

    def __init__(self, P, Q, lr):
        self.P, self.Q, self.lr = P, Q, float(lr)

    def P_rows_new64(self):
        return self.P[self.urows].to(torch.float64) - self.lr * self.gP.to(torch.float64)      # integer x 2^-k: exact

    def Q_rows_new64(self):
        return self.Q[self.irows].to(torch.float64) - self.lr * self.gQ.to(torch.float64)

    def P_rows_new(self):
        """float32 rows of the updated user table at `urows` (the other rows keep their bits)"""
        return self.P_rows_new64().to(torch.float32)

    def Q_rows_new(self):
        return self.Q_rows_new64().to(torch.float32)

    def P_new(self):
        return self.P.to(torch.float32).index_copy_(0, self.urows, self.P_rows_new())

    def Q_new(self):
        return self.Q.to(torch.float32).index_copy_(0, self.irows, self.Q_rows_new())

    @staticmethod
    def dense(rows, vals, n):
        """float32 [n, ...] with vals at `rows`, zero elsewhere"""
        out = torch.zeros((n,) + tuple(vals.shape[1:]), dtype=torch.float32, device=vals.device)
        return out.index_copy_(0, rows, vals.to(torch.float32))


def exact_step(P, Q, u, i, j, loss, lr, biases=None, device="cpu"):
    """mf_sgd_step with reg_1 = reg_2 = 0 on integer tables, in int64.  HL (loss.py:20-23): m = 1 - (pos - neg), the sample
    is active when m >= 0 (pair_coef, common.h), coefficients (-1, +1).  SL: j holds the labels, coefficient 2 (pos - y).
    biases = (u_bias, i_bias, bias) of FM (integers): added to the scores (FMRecommender.py:61-68).
    Plain torch integer arithmetic (gathers, products, index_add_) on `device`: numpy arrays or tensors go in, int64
    tensors that were prepared once (tables shared by many steps) are used as they are."""
    Pi, Qi = _int_tensor(P, "P", device), _int_tensor(Q, "Q", device)
    u, i, j = (_int_tensor(x, "ids", device) for x in (u, i, j))
    d = Pi.shape[1]
    pmax, qmax = _rowmax(Pi), _rowmax(Qi)
    pu, qi = Pi[u], Qi[i]
    pos = (pu * qi).sum(1)
    bound = d * pmax[u] * qmax[i]
    bterm = lambda it: 0
    if biases is not None:
        bu, bi, b0 = (_int_tensor(x, "bias", device).reshape(-1) for x in biases)
        bterm = lambda it: bu[u] + bi[it] + b0[0]
        bound = bound + bu[u].abs() + bi.abs().max() + b0[0].abs()
    pos = pos + bterm(i)
    st = ExactStep(Pi, Qi, lr)
    st.urows, inv_u = torch.unique(u, return_inverse=True)
    nu = len(st.urows)
    if loss == HL:
        qj = Qi[j]
        neg = (pu * qj).sum(1) + bterm(j)
        bound = bound + d * pmax[u] * qmax[j] + 1                     # bounds pos, neg, pos - neg and m
        m = 1 - (pos - neg)
        act = (m >= 0).to(torch.int64)
        terms = m.clamp(min=0)
        st.gP = _segment_sum(inv_u, nu, act[:, None] * (qj - qi))     # cp q_i + cn q_j = act (q_j - q_i)
        st.aP = _segment_sum(inv_u, nu, act * (qmax[i] + qmax[j]))
        apu = act[:, None] * pu
        st.irows, inv_i = torch.unique(torch.cat([i, j]), return_inverse=True)
        ni = len(st.irows)
        st.gQ = _segment_sum(inv_i, ni, torch.cat([-apu, apu]))
        st.aQ = _segment_sum(inv_i, ni, (act * pmax[u]).repeat(2))
        st.g_i_bias = _segment_sum(inv_i, ni, torch.cat([-act, act]))
        st.a_i_bias = _segment_sum(inv_i, ni, act.repeat(2))
    elif loss == SL:
        bound = bound + j.abs()
        e = pos - j
        c = 2 * e
        terms = e * e
        st.gP = _segment_sum(inv_u, nu, c[:, None] * qi)
        st.aP = _segment_sum(inv_u, nu, c.abs() * qmax[i])
        st.irows, inv_i = torch.unique(i, return_inverse=True)
        ni = len(st.irows)
        st.gQ = _segment_sum(inv_i, ni, c[:, None] * pu)
        st.aQ = _segment_sum(inv_i, ni, c.abs() * pmax[u])
        st.g_i_bias = _segment_sum(inv_i, ni, c)
        st.a_i_bias = _segment_sum(inv_i, ni, c.abs())
    else:
        raise NotImplementedError(f"exact_step: loss {loss}")
    st.abs_score = int(bound.max())
    st.loss = int(terms.sum())
    st.abs_loss = int(terms.abs().sum())
    st.abs_term = int(terms.abs().max())
    return st


def assert_exact_domain(st):
    """Order-independence as a checked condition.  For every updated row, (|w| + lr sum |term|) / lr < 2^24: w and every
    partial sum of lr x terms are multiples of lr below 2^24 lr, so any partial sum in any order is an fp32 number.  The
    same for the raw gradients (sum |term| < 2^24), the bias gradient, the scores and the loss (the sum of the terms fits
    fp32 even where a kernel adds them in fp32 before widening).  And the reference itself survives the float32 round
    trip."""
    inv = 1.0 / st.lr
    assert inv == int(inv) and int(inv) & (int(inv) - 1) == 0, f"lr {st.lr} is not a power of two"
    for W, rows, a, g, what in ((st.P, st.urows, st.aP, st.gP, "P"), (st.Q, st.irows, st.aQ, st.gQ, "Q")):
        assert int(a.max()) < EXACT_CAP, f"g{what}: sum of |terms| {int(a.max())} >= 2^24"
        bound = _rowmax(W[rows]) * int(inv) + a
        assert int(bound.max()) < EXACT_CAP, f"{what}: (|w| + lr sum |terms|) / lr = {int(bound.max())} >= 2^24"
        assert bool((_rowmax(g) <= a).all()), f"g{what}: a row exceeds its own bound"
    assert int(st.a_i_bias.max()) < EXACT_CAP, "g_i_bias: sum of |coefficients| >= 2^24"
    assert st.abs_score < EXACT_CAP, f"scores: sum of |p||q| {st.abs_score} >= 2^24"
    assert st.abs_term < EXACT_CAP and st.abs_loss < EXACT_CAP, f"loss: sum of |terms| {st.abs_loss} >= 2^24"
    for x in (st.P_rows_new64(), st.Q_rows_new64(), st.gP.to(torch.float64), st.gQ.to(torch.float64),
              st.g_i_bias.to(torch.float64), torch.tensor(float(st.loss), dtype=torch.float64)):
        assert torch.equal(x.to(torch.float32).to(torch.float64), x), "the reference does not fit fp32"


# ----------------------------------------------------------------------------------------------------------------------
# what the GPU test runs (the host test checks the domain of every one of these without a GPU)
# ----------------------------------------------------------------------------------------------------------------------
D_ALL = (32, 64, 128, 256,          # the exact shapes of dispatch_d
         20, 48, 100, 200, 300,     # d % 4 == 0
         7, 130, 257,               # the scalar-width shapes
         512)                       # the upper limit
D_SL = (20, 64, 257)
B_MAIN = 4096
B_SMALL = (1, 2, 129, 256)
OFF_GRID = {1: 1, 129: 128, 2049: 2048}        # B -> the period nearest to it
D_OFF_GRID = (64, 256, 300)
B_LONG, D_LONG = 32768, (64, 300)


def _pair(lu, li):
    """item layouts paired with user layouts index by index (the shorter list wraps)"""
    n = max(len(lu), len(li))
    return [(f"{lu[k % len(lu)][0]}|{li[k % len(li)][0]}", lu[k % len(lu)][1], li[k % len(li)][1]) for k in range(n)]


def main_cases(pointwise):
    """B = 4096: user layout k with item layout k, plus four crossed pairs - a hot row on one side over many rows on the
    other (a batch whose items are all one item has pos == neg in every sample: its user gradient is zero whatever is
    summed)"""
    B, E = B_MAIN, (B_MAIN if pointwise else 2 * B_MAIN)
    cases = _pair(list(layouts(B)), list(layouts(E)))
    for nu, ni in (("one", "period(4,1)"), ("period(4,1)", "one"), ("long(3)", "comb(1,7)"), ("comb(1,7)", "long(3)")):
        cases.append((f"{nu}|{ni}", named(B, nu), named(E, ni)))
    return cases


def small_cases(B):
    return _pair(list(layouts(B, max_p=256)), list(layouts(2 * B, max_p=256)))


def off_grid_cases(B):
    p = OFF_GRID[B]
    out = []
    for lead in sorted({0, 1, p - 1}):
        for pi in (p, 2 * p):
            lu, li = period(B, p, lead) or [B], period(2 * B, pi, lead) or [2 * B]
            out.append((f"period({p},{lead})|period({pi},{lead})", lu, li))
    return out


def long_cases():
    """a hot row through several kEdgeBlock blocks of chunks on either side, alone and together"""
    B = B_LONG
    return [("period(8,1)|long(3)", named(B, "period(8,1)"), named(2 * B, "long(3)")),
            ("long(3)|period(8,1)", named(B, "long(3)"), named(2 * B, "period(8,1)")),
            ("long(3)|long(3)", named(B, "long(3)"), named(2 * B, "long(3)"))]


def make_batch(case, loss, seed):
    """(u, i, j, user_num, item_num) of one (name, layout_u, layout_i): it does not depend on d"""
    _, lu, li = case
    return batch(lu, li, np.random.default_rng(seed), pointwise=(loss == SL))


def make_biases(user_num, item_num, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(-2, 3, user_num).astype(np.float32), rng.integers(-2, 3, item_num).astype(np.float32),
            np.array([1.0], np.float32))


def make_case(case, d, loss, seed, biases=False):
    """(u, i, j, P, Q, biases or None, ExactStep) of one case with tables of its own"""
    u, i, j, U, I = make_batch(case, loss, seed)
    P, Q = int_tables(np.random.default_rng(seed + 7), U, I, d, loss)
    b = make_biases(U, I, seed + 1) if biases else None
    return u, i, j, P, Q, b, exact_step(P, Q, u, i, j, loss, LR[loss], biases=b)
