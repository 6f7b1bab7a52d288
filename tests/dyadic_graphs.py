"""Graphs on which the normalised adjacency D^-1/2 A D^-1/2 is exact in fp32 - pure numpy, no GPU.

In a bipartite component where every user has degree a and every item degree b with a * b = 4^k and a, b >= 4, the
stored coefficient  float32((a + 1e-7)^-1/2 * (b + 1e-7)^-1/2)  is exactly 2^-k: it falls short of 2^-k by the relative
0.5e-7 * (1 / a + 1 / b), which for a, b >= 4 stays under the half-ulp 2^-25 just below a power of two (the tightest
pair, (4, 4), uses 0.84 of it).  With small-integer X and node-dropout scales 2 and 4 (p = 0.5, 0.75) every term of a
row is an integer multiple of the row's coefficient, and as long as the sum of their magnitudes stays below 2^24 such
units (`assert_exact_domain`, checked for every case before it runs) every partial sum in any order is an fp32 number:
a product that adds every entry exactly once returns the reference's bits, and one entry dropped, doubled, masked by
the wrong index or sent to the wrong row does not.

`biregular` builds such a graph from (user degree, item degree, users) components, `irregular` one with stated row
lengths for the round-off tests (its coefficients are no powers of two).
"""
import numpy as np

EXACT_CAP = 1 << 24

# (user degree a, item degree b, users): a * b is a power of 4.  Rows of exactly 256 entries (one segment of the NGCF
# product, written directly), of 512 and of 1024 entries (2 and 4 segments) on the user side and on the item side.
DEFAULT_COMPONENTS = ((1024, 4, 4), (4, 1024, 1024), (8, 512, 512), (512, 8, 8), (16, 256, 256), (256, 16, 16),
                      (4, 4, 8), (4, 16, 16), (8, 8, 8), (16, 16, 16), (4, 64, 64), (64, 64, 64), (32, 8, 8), (32, 32, 32))
DEFAULT_DEGREES = (0, 4, 8, 16, 32, 64, 256, 512, 1024)

IRREGULAR_LENGTHS = (0, 1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 300, 511, 512, 513, 769, 1000)


def biregular(components=DEFAULT_COMPONENTS, gap=1):
    """(users int32[E], items int32[E], U, I, spans): component (a, b, nu) has E = nu * a links over nu users and
    ni = E / b items, link e joining user u0 + e // a to item i0 + e % ni - a <= ni consecutive items per user, so the
    pairs are distinct, and every item is met E / ni = b times.  `gap` isolated users and items lie before the first
    component, between two components and after the last: row 0 and the last row of the user block and of the item block
    are isolated.  spans[k] = (u0, nu, i0, ni) of component k."""
    assert gap >= 1
    gu, gi, spans = [], [], []
    u0 = i0 = gap
    for a, b, nu in components:
        E = nu * a
        ni = E // b
        if ni * b != E or a > ni:
            raise ValueError(f"component {(a, b, nu)}: {E} links do not give items of degree {b} with {a} <= {ni} items")
        e = np.arange(E, dtype=np.int64)
        gu.append(u0 + e // a)
        gi.append(i0 + e % ni)
        spans.append((u0, nu, i0, ni))
        u0 += nu + gap
        i0 += ni + gap
    return np.concatenate(gu).astype(np.int32), np.concatenate(gi).astype(np.int32), int(u0), int(i0), spans


def irregular(lengths=IRREGULAR_LENGTHS):
    """(users, items, U, I): user u is linked to lengths[u] distinct items, (start_u * 7 + t) mod I for t < lengths[u]
    with I larger than the longest row - the construction of _layout_graph in test_gpu_segment_layouts.py.  Swapping the
    roles of users and items puts the long rows into the second half of the entry list."""
    lens = np.asarray(lengths, np.int64)
    I = int(lens.max()) + 37
    gu = np.repeat(np.arange(len(lens)), lens)
    start = np.cumsum(lens) - lens
    t = np.arange(len(gu)) - start[gu]
    gi = (start[gu] * 7 + t) % I
    return gu.astype(np.int32), gi.astype(np.int32), len(lens), I


def _is_pow2(v):
    m, _ = np.frexp(np.asarray(v, np.float64))
    return m == 0.5


def assert_exact_domain(val, X, scale, prefill=None, halved=False):
    """Order-independence as a checked condition, for  prefill + scale * (A X)  and its transpose (A is symmetric in
    structure and in value, so the row-wise check covers both).

    val: the read-back entries (row, col, val) of the graph.  Raises unless every coefficient is a power of two, each row
    has ONE coefficient c_r, `scale` is a power of two and X and the prefill are integers, and unless
        max|X| * rowlen_r * scale  +  max_r|prefill| / c_r  <  2^24
    for every row r: every term is an integer multiple of c_r, and every partial sum in any order stays below 2^24 such
    units.  halved: the sum is halved at the end ((X + A X) / 2) and then added to integers (dE0 + ... / 2) - the unit is
    c_r / 2, so the bound doubles."""
    row, col, v = (np.asarray(t) for t in val)
    X = np.asarray(X, np.float64)
    N = X.shape[0]
    if not (len(row) == len(col) == len(v) and len(v) > 0 and row.min() >= 0 and max(row.max(), col.max()) < N):
        raise AssertionError("entries outside the matrix")
    if not (_is_pow2(v).all() and (v > 0).all()):
        bad = v[~_is_pow2(v)]
        raise AssertionError(f"{len(bad)} coefficients are no powers of two, the first of them {bad[0]!r}")
    if not (_is_pow2(scale) and scale >= 1):
        raise AssertionError(f"scale {scale!r} is no power of two")
    if not np.array_equal(X, np.rint(X)):
        raise AssertionError("X holds values that are no integers")
    rowlen = np.bincount(row, minlength=N)
    lo = np.full(N, np.inf)
    hi = np.zeros(N)
    np.minimum.at(lo, row, v)
    np.maximum.at(hi, row, v)
    used = rowlen > 0
    if not np.array_equal(lo[used], hi[used]):
        raise AssertionError(f"{int((lo[used] != hi[used]).sum())} rows have more than one coefficient")
    bound = np.abs(X).max() * rowlen.astype(np.float64) * float(scale)
    if prefill is not None:
        P = np.asarray(prefill, np.float64)
        if not np.array_equal(P, np.rint(P)):
            raise AssertionError("the prefill holds values that are no integers")
        pmax = np.abs(P).reshape(N, -1).max(1)
        bound = bound + pmax / np.where(used, hi, 1.0)
    if halved:
        bound = bound * 2
    if not bound.max() < EXACT_CAP:
        r = int(bound.argmax())
        raise AssertionError(f"row {r}: {bound[r]:.0f} units of its coefficient >= 2^24")
