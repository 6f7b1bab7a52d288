"""The graph products of NGCF and LightGCN (csrc/lightgcn.hip, segsum.hip) bit for bit against exact dyadic sums.

tests/dyadic_graphs.py builds a graph of biregular components whose normalised adjacency holds powers of two only
(tests/test_host_dyadic_graphs.py checks that without a GPU).  With small-integer X, node-dropout scales 2 and 4 and the
domain CHECKED by `assert_exact_domain` before anything runs, every partial sum in any order is an fp32 number: a product
that adds every entry exactly once returns the bits of the fp64 scipy product, and one entry dropped, doubled, masked by
the wrong index or sent to the wrong row does not.  The graph has rows of 4 ... 64, of exactly 256 (one segment of
daisy_lgcn_spmm_ex, written directly), of 512 and of 1024 entries (2 and 4 segments through seg_part and
k_lg_spmm_join) among the users and among the items, and isolated rows at both ends of either block.

a / b  daisy_lgcn_spmm_ex in each of its launch forms (k_lg_spmm_seg<8 | 16 | 32 | 64, true>, the last in one and in two
       column passes, and <64, false> for widths that are no multiple of 4 and for pitches / pointers that rule the
       float4 loads out): plain, masked, masked transpose, accumulate, accumulate masked transpose.  X and out are
       views into wider buffers filled with a NaN bit pattern; the WHOLE buffers are compared, so nothing is written
       outside the view, isolated rows come back +0 over a NaN prefill (and unchanged with accumulate), and a second
       call returns the same bits.
c      LightGCN's products on the same graph: graph.spmm, spmm_rows over row ranges, propagate and backprop in both
       set_reproducible modes.  (Every degree of a dyadic graph is even, so every row range holds an even number of
       entries: the borrowed entry of an odd range stays with test_gpu_lightgcn_dist.py.)
d      Row lengths 0 ... 1000 around every segment size (`irregular` and its twin with the long rows last): these
       coefficients are no powers of two, so the comparison is with the fp64 product at a DERIVED bound,
       |got - want| <= 1.01 k u S with u = 2^-24, S = (|A_drop| |X|)[r, c] (+ |prefill|) and
       k = min(len, 256) + 6 + ceil(len / 256) + 2: the longest fma chain of a segment, the butterfly, the join adds,
       one rounding of the scale and one accumulate add; the 1 % covers 1 / (1 - k u).  A missing entry of the
       1000-entry row moves it by about 1e-3 S; the bound there is 1.6e-5 S.
e      ops.csr_row_sum and ops.axpby on integers, exact.

Each test prints the number of (form, case) pairs it compared.
"""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import dyadic_graphs as DG
from oracle import lightgcn_numpy as LG
from oracle import neumf_numpy as NM

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0x7FC5A5A5                 # a NaN with a payload: read by mistake it poisons the sum, overwritten it shows
SEED = (2022 << 32) | 7           # NGCF's seeds carry the model seed in the upper word
D_MAX = 512
LG_D = (64, 130, 160, 256, 300, 512)
P_IRR = 0.3


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _f32(x64, what):
    """an fp64 reference as fp32, after checking that nothing is lost; -0 becomes +0"""
    y = (x64 + 0.0).astype(np.float32)
    assert np.array_equal(y.astype(np.float64), x64), f"{what}: the reference does not fit fp32"
    return y


def _bits(t):
    return t.view(torch.int32)


class Failures(list):
    """collects mismatches so that one run names every (form, case) that misses, not the first only"""

    def same(self, got, want, what):
        """bit for bit, NaN patterns and the sign of zero included"""
        got, want = _bits(got) if got.dtype == torch.float32 else got, _bits(want) if want.dtype == torch.float32 else want
        assert got.shape == want.shape, (what, got.shape, want.shape)
        if torch.equal(got, want):
            return
        g2, w2 = got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
        bad = (g2 != w2).any(1).nonzero().reshape(-1)
        r = int(bad[0])
        c = int((g2[r] != w2[r]).nonzero()[0])
        self.append(f"{what}: {len(bad)} rows differ; row {r} column {c}: got "
                    f"{g2[r, c:c + 4].view(torch.float32).tolist()} want {w2[r, c:c + 4].view(torch.float32).tolist()}")

    def done(self, n, label):
        print(f"\ngraph products: {label}: {n} (form, case) pairs")
        assert not self, f"{len(self)} mismatches, the first of them:\n" + "\n".join(self[:12])


class Strided:
    """a float32 view [N, d] at column `col` of an int32 buffer [N + 2, pitch] that holds the sentinel everywhere else:
    one guard row above and below, pitch - d guard columns"""

    def __init__(self, N, d, pitch=None, col=0):
        pitch = d if pitch is None else pitch
        assert col + d <= pitch
        self.col = col
        self.buf = torch.full((N + 2, pitch), SENT, dtype=torch.int32, device=DEV)
        self.bits = self.buf[1:N + 1, col:col + d]
        self.view = self.bits.view(torch.float32)
        assert self.view.stride(0) == pitch or d == pitch

    def set(self, t):
        self.bits.copy_(_bits(t))
        return self

    def expect(self, t):
        """the whole buffer as it has to look when the view holds t and nothing else was touched"""
        exp = torch.full_like(self.buf, SENT)
        exp[1:-1, self.col:self.col + t.shape[1]] = _bits(t)
        return exp


def _vec(x, y):
    """the condition under which daisy_lgcn_spmm_ex takes a float4 kernel"""
    d = x.view.shape[1]
    ldx, ldy = max(x.view.stride(0), d), max(y.view.stride(0), d)
    return d % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 and x.view.data_ptr() % 16 == 0 and y.view.data_ptr() % 16 == 0


# ----------------------------------------------------------------------------------------------------------------------
# the dyadic graph, its masks and the host references, once per module
# ----------------------------------------------------------------------------------------------------------------------
class World:
    def __init__(self):
        from daisyrec_amd import ops
        self.ops = ops
        gu, gi, U, I, self.spans = DG.biregular()
        self.U, self.I, self.N = U, I, U + I
        N = self.N
        self.graph = ops.LgcnGraph(_dev(gu), _dev(gi), U, I)
        row, col, val = (t.cpu().numpy() for t in self.graph.coo())
        indptr, ocol, oval = LG.norm_adj_csr(gu, gi, U, I)
        assert self.graph.nnz == len(oval) == 61248
        assert np.array_equal(row, np.repeat(np.arange(N), np.diff(indptr))) and np.array_equal(col, ocol)
        assert np.array_equal(val.view(np.uint32), oval.view(np.uint32))        # exact here, not within 1 ulp
        self.coo, self.indptr = (row, col, val), indptr
        nnz = len(val)
        self.keep = {}
        for p in (0.5, 0.75):
            k = NM.drop_keep(SEED, ops.NGCF_NODE_STREAM, np.arange(nnz), p)
            assert np.array_equal(ops.dropout_mask(SEED, ops.NGCF_NODE_STREAM, nnz, p).cpu().numpy().astype(bool), k)
            self.keep[p] = k

        def csr(p):
            w = val.astype(np.float64) if p == 0 else np.where(self.keep[p], val.astype(np.float64) / (1 - p), 0.0)
            return sp.csr_matrix((w, (row, col)), shape=(N, N))

        rng = np.random.default_rng(20)
        X = rng.integers(-8, 9, (N, D_MAX)).astype(np.float64)
        pre = rng.integers(-8, 9, (N, D_MAX)).astype(np.float64)
        for scale, pf in ((1.0, None), (2.0, None), (4.0, None), (1.0, pre), (4.0, pre)):
            DG.assert_exact_domain(self.coo, X, scale, prefill=pf)
        A0, A2, A4t = csr(0), csr(0.5), csr(0.75).T.tocsr()
        plain, half, quart_t = A0 @ X, A2 @ X, A4t @ X
        self.X, self.pre = _dev(_f32(X, "X")), _dev(_f32(pre, "prefill"))
        # (name, arguments of spmm_ex, the view's contents before the call (None: NaN), expected contents)
        self.cases = [
            ("plain", dict(), None, _dev(_f32(plain, "A X"))),
            ("keep 0.5", dict(keep=(0.5, SEED)), None, _dev(_f32(half, "A_drop X"))),
            ("keep 0.75 transposed", dict(keep=(0.75, SEED), transpose=True), None, _dev(_f32(quart_t, "A_drop^T X"))),
            ("accumulate", dict(accumulate=True), self.pre, _dev(_f32(pre + plain, "prefill + A X"))),
            ("accumulate keep 0.75 transposed", dict(accumulate=True, keep=(0.75, SEED), transpose=True), self.pre,
             _dev(_f32(pre + quart_t, "prefill + A_drop^T X"))),
        ]
        deg = np.diff(indptr)
        self.isolated = _dev(np.flatnonzero(deg == 0))
        assert deg[0] == deg[U - 1] == deg[U] == deg[N - 1] == 0
        # LightGCN: X in [-4, 4] so that the halved sums of propagate and backprop stay exact
        X4 = rng.integers(-4, 5, (N, D_MAX)).astype(np.float64)
        dE0 = rng.integers(-8, 9, (N, D_MAX)).astype(np.float64)
        DG.assert_exact_domain(self.coo, X4, 1.0)
        DG.assert_exact_domain(self.coo, X4, 1.0, prefill=np.abs(X4), halved=True)                       # (X + A X) / 2
        DG.assert_exact_domain(self.coo, X4, 1.0, prefill=np.abs(X4) + 2 * np.abs(dE0), halved=True)     # dE0 + (G + A G) / 2
        AX4 = A0 @ X4
        self.X4, self.dE0, self.AX4 = _dev(_f32(X4, "X4")), _dev(_f32(dE0, "dE0")), _dev(_f32(AX4, "A X4"))
        self.prop = _dev(_f32((X4 + AX4) / 2, "(X + A X) / 2"))
        self.back = _dev(_f32(dE0 + (X4 + AX4) / 2, "dE0 + (G + A G) / 2"))

    def close(self):
        self.graph.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


# ----------------------------------------------------------------------------------------------------------------------
# a / b: daisy_lgcn_spmm_ex, every launch form
# ----------------------------------------------------------------------------------------------------------------------
def _form(d, xpitch=None, xcol=0, ypitch=None, ycol=0):
    return d, xpitch, xcol, ypitch, ycol


# row of the table -> (float4 kernel expected, lanes per row, column passes, [(d, X pitch, X column, out pitch, out column)])
SPMM_EX_FORMS = {
    "<8, true>": (True, 8, 1, [_form(4), _form(20), _form(32)]),
    "<16, true>": (True, 16, 1, [_form(36), _form(64), _form(64, 132, 36, 132, 36)]),
    "<32, true>": (True, 32, 1, [_form(68), _form(128)]),
    "<64, true> one pass": (True, 64, 1, [_form(132), _form(256)]),
    "<64, true> two passes": (True, 64, 2, [_form(260), _form(512)]),
    "<64, false> d % 4 != 0": (False, 64, None, [_form(d) for d in (1, 7, 63, 65, 130, 511)]),
    # an odd pitch on both sides; X at column 2 of a pitch-72 buffer (pitches and `out` fit, the pointer is 8 bytes off);
    # only `out` at an odd pitch
    "<64, false> layout": (False, 64, 1, [_form(64, 69, 3, 69, 3), _form(64, 72, 2, 72, 4), _form(64, None, 0, 69, 0)]),
}


def _lanes(d):
    return 8 if d <= 32 else 16 if d <= 64 else 32 if d <= 128 else 64


FORM_IDS = ["vec8", "vec16", "vec32", "vec64_one_pass", "vec64_two_passes", "scalar_by_width", "scalar_by_layout"]


@pytest.mark.parametrize("row", list(SPMM_EX_FORMS), ids=FORM_IDS)
def test_spmm_ex_exact_in_every_launch_form(world, row):
    w, fails, n = world, Failures(), 0
    want_vec, lanes, passes, forms = SPMM_EX_FORMS[row]
    for d, xp, xc, yp, yc in forms:
        x = Strided(w.N, d, xp, xc).set(w.X[:, :d])
        x_before = x.buf.clone()
        y = Strided(w.N, d, yp, yc)
        # the table's row is the kernel this layout reaches
        assert _vec(x, y) == want_vec, (row, d)
        if want_vec:
            assert _lanes(d) == lanes and -(-d // (lanes * 4)) == passes, (row, d)
        if row.endswith("layout"):
            assert d % 4 == 0
        name = f"{row} d={d} X[{xp or d}:{xc}] out[{yp or d}:{yc}]"
        for case, kw, before, after in w.cases:
            def prefill():
                if before is None:
                    y.view.fill_(float("nan"))
                else:
                    y.set(before[:, :d])
            exp = y.expect(after[:, :d])
            prefill()
            w.graph.spmm_ex(x.view, out=y.view, **kw)
            fails.same(y.buf, exp, f"{name} {case}")
            # isolated rows: +0 over the NaN prefill, unchanged under accumulate (part of `exp`; spelled out)
            iso = y.view[w.isolated]
            iso_want = torch.zeros_like(iso) if before is None else before[w.isolated, :d]
            fails.same(iso.contiguous(), iso_want.contiguous(), f"{name} {case}: isolated rows")
            if kw.get("accumulate"):
                prefill()
            w.graph.spmm_ex(x.view, out=y.view, **kw)
            fails.same(y.buf, exp, f"{name} {case}: second call")
            fails.same(x.buf, x_before, f"{name} {case}: X")
            n += 1
    fails.done(n, f"spmm_ex {row}")


# ----------------------------------------------------------------------------------------------------------------------
# c: LightGCN's products on the same graph
# ----------------------------------------------------------------------------------------------------------------------
def _row_ranges(w):
    """the blocks of worlds 1, 3 and 8, and ranges that begin and end between two rows of 1024 entries"""
    N, out = w.N, []
    for world in (1, 3, 8):
        rows = (N + world - 1) // world
        out += [(min(r * rows, N), min((r + 1) * rows, N), rows) for r in range(world)]
    (u0, nu, _, _), (_, _, i1, ni1) = w.spans[0], w.spans[1]
    assert nu == 4 and ni1 == 4 and (np.diff(w.indptr)[[u0 + 1, w.U + i1 + 1]] == 1024).all()
    for lo, hi in ((u0 + 1, u0 + 3), (u0 + 2, w.U + i1 + 2), (w.U + i1 + 1, w.U + i1 + 3)):
        out.append((lo, hi, hi - lo))
    return out


@pytest.mark.parametrize("d", LG_D)
def test_lightgcn_products_exact(world, d):
    w, g, fails, n = world, world.graph, Failures(), 0
    X, want = w.X4[:, :d].contiguous(), w.AX4[:, :d].contiguous()
    x_before = X.clone()
    guard = 3
    try:
        for repro in (False, True):
            g.set_reproducible(repro)
            tag = f"d={d} reproducible={repro}"
            fails.same(g.spmm(X), want, f"spmm {tag}")
            n += 1
            for lo, hi, rows in _row_ranges(w):
                big = torch.full((rows + 2 + 2 * guard, d), SENT, dtype=torch.int32, device=DEV)
                blk = big[guard:guard + rows + 2].view(torch.float32)
                own = g.spmm_rows(X, blk, lo, hi)
                fails.same(own, want[lo:hi], f"spmm_rows [{lo}, {hi}) {tag}")
                rest = torch.cat([big[:guard], big[guard + 2 + hi - lo:]])            # beyond the two spare rows
                fails.same(rest, torch.full_like(rest, SENT), f"spmm_rows [{lo}, {hi}) {tag}: guard rows")
                n += 1
            fails.same(g.propagate(X, 1), w.prop[:, :d].contiguous(), f"propagate {tag}")
            dE0 = w.dE0[:, :d].clone()                                   # a copy at d = 512 too: backprop adds in place
            g.backprop(X, 1, dE0)
            fails.same(dE0, w.back[:, :d].contiguous(), f"backprop {tag}")
            fails.same(X, x_before, f"X after {tag}")
            n += 2
    finally:
        g.set_reproducible(False)
    fails.done(n, f"lightgcn d={d}")


# ----------------------------------------------------------------------------------------------------------------------
# d: irregular row lengths at the derived round-off bound
# ----------------------------------------------------------------------------------------------------------------------
IRR_FORMS = [_form(20), _form(36), _form(68), _form(132), _form(260), _form(65), _form(64, 69, 3, 69, 3)]


@pytest.mark.parametrize("twin", [False, True], ids=["long_rows_first", "long_rows_last"])
def test_spmm_ex_irregular_rows_within_the_derived_bound(twin):
    from daisyrec_amd import ops
    gu, gi, U, I = DG.irregular()
    if twin:
        gu, gi, U, I = gi, gu, I, U
    N, dmax = U + I, max(f[0] for f in IRR_FORMS)
    graph = ops.LgcnGraph(_dev(gu), _dev(gi), U, I)
    row, col, val = (t.cpu().numpy() for t in graph.coo())
    nnz = len(val)
    lens = np.bincount(row, minlength=N)
    assert np.array_equal(lens[U:] if twin else lens[:U], DG.IRREGULAR_LENGTHS)
    keep = NM.drop_keep(SEED, ops.NGCF_NODE_STREAM, np.arange(nnz), P_IRR)
    assert np.array_equal(ops.dropout_mask(SEED, ops.NGCF_NODE_STREAM, nnz, P_IRR).cpu().numpy().astype(bool), keep)
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(P_IRR)))              # the kernel's fp32 scale
    A = sp.csr_matrix((val.astype(np.float64), (row, col)), shape=(N, N))
    Ad = sp.csr_matrix((np.where(keep, val.astype(np.float64) * scale, 0.0), (row, col)), shape=(N, N))
    rng = np.random.default_rng(int(twin))
    X = rng.integers(1, 5, (N, dmax)).astype(np.float64)                                # nothing cancels: S = the product
    pre = rng.integers(1, 5, (N, dmax)).astype(np.float64)
    k = np.minimum(lens, 256) + 6 + -(-lens // 256) + 2
    unit = 1.01 * k[:, None] * 2.0 ** -24
    plain, masked, masked_t = A @ X, Ad @ X, Ad.T.tocsr() @ X
    cases = [("plain", dict(), None, plain, plain), ("keep 0.3", dict(keep=(P_IRR, SEED)), None, masked, masked),
             ("keep 0.3 transposed", dict(keep=(P_IRR, SEED), transpose=True), None, masked_t, masked_t),
             ("accumulate", dict(accumulate=True), pre, pre + plain, pre + plain)]
    Xd, pred = _dev(X.astype(np.float32)), _dev(pre.astype(np.float32))
    worst, n, misses = 0.0, 0, []
    for d, xp, xc, yp, yc in IRR_FORMS:
        x = Strided(N, d, xp, xc).set(Xd[:, :d])
        for case, kw, before, want, S in cases:
            y = Strided(N, d, yp, yc)
            if before is None:
                y.view.fill_(float("nan"))
            else:
                y.set(pred[:, :d])
            graph.spmm_ex(x.view, out=y.view, **kw)
            got = y.view.cpu().numpy().astype(np.float64)
            y.bits.fill_(SENT)
            assert bool((y.buf == SENT).all()), f"d={d} {case}: written outside the view"
            err, bound = np.abs(got - want[:, :d]), unit * S[:, :d]
            ok = err <= bound                                                            # a NaN fails
            ratio = float(np.nanmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
            worst = max(worst, ratio)
            if not ok.all():
                r, c = np.argwhere(~ok)[0]
                misses.append(f"d={d} {case}: {int((~ok).sum())} elements beyond the bound; row {r} (length {lens[r]}) "
                              f"column {c}: got {got[r, c]!r} want {want[r, c]!r} bound {bound[r, c]:.3e}")
            n += 1
    graph.close()
    print(f"\ngraph products: irregular rows, long rows {'last' if twin else 'first'}: {n} (form, case) pairs, "
          f"largest error / bound {worst:.3f}")
    assert not misses, "\n".join(misses[:12])


# ----------------------------------------------------------------------------------------------------------------------
# e: the small neighbours
# ----------------------------------------------------------------------------------------------------------------------
CSR_LENGTHS = (0, 1, 2, 17, 300, 5000)
CSR_D = (1, 16, 17, 64, 100)


def test_csr_row_sum_exact():
    """one lane group per row, 16 rows per workgroup: 24 rows (every length four times, shuffled) make two workgroups"""
    from daisyrec_amd import ops
    rng = np.random.default_rng(5)
    lens = rng.permutation(np.repeat(CSR_LENGTHS, 4))
    R, M = len(lens), 6000
    indptr = np.zeros(R + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    cols = rng.integers(0, M, int(indptr[-1])).astype(np.int32)
    cols[indptr[np.flatnonzero(lens == 5000)[0]]] = M - 1                        # the last row of X is read
    X = rng.integers(-8, 9, (M, max(CSR_D))).astype(np.float64)
    assert 8 * lens.max() < DG.EXACT_CAP
    want = _f32(sp.csr_matrix((np.ones(len(cols)), cols, indptr), shape=(R, M)) @ X, "row sums")
    Xd, wd, ip, cd = _dev(X.astype(np.float32)), _dev(want), _dev(indptr), _dev(cols)
    empty = _dev(np.flatnonzero(lens == 0))
    fails = Failures()
    for d in CSR_D:
        out = Strided(R, d)
        exp = out.expect(wd[:, :d])
        exp[1 + empty] = SENT                                                    # rows without entries keep their contents
        ops.csr_row_sum(ip, cd, Xd[:, :d].contiguous(), out.view)
        fails.same(out.buf, exp, f"csr_row_sum d={d}")
    fails.done(len(CSR_D), "csr_row_sum")


@pytest.mark.parametrize("n", [1, 1023, 1024 * 4 * 256 + 3])
def test_axpby_exact(n):
    from daisyrec_amd import ops
    rng = np.random.default_rng(n)
    x0 = rng.integers(-100, 101, n).astype(np.float32)
    y0 = rng.integers(-100, 101, n).astype(np.float32)
    guard, count = 4, 0
    for a, b in ((3, -2), (-1, 4)):
        for zero_x in (False, True):
            bufs = [torch.full((n + 2 * guard,), SENT, dtype=torch.int32, device=DEV) for _ in range(2)]
            x, y = (t[guard:guard + n].view(torch.float32) for t in bufs)
            x.copy_(_dev(x0))
            y.copy_(_dev(y0))
            ops.axpby(x, a, b, y, zero_x=zero_x)
            what = f"n={n} a={a} b={b} zero_x={zero_x}"
            assert torch.equal(y, _dev(a * x0 + b * y0)), what
            assert torch.equal(x, torch.zeros_like(x) if zero_x else _dev(x0)), what        # zeroed only when asked
            for t in bufs:
                assert bool((t[:guard] == SENT).all()) and bool((t[guard + n:] == SENT).all()), what
            count += 1
    print(f"\ngraph products: axpby n={n}: {count} (form, case) pairs")
