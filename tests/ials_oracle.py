"""iALS in numpy fp64: the statement the HIP kernels of csrc/ials.hip are checked against.

A half-sweep solves, for every row u of a CSR (row_ptr, col, val) against the other side's table Y [n, d],

    A_u x_u = b_u,   A_u = Y^T Y + reg I + sum_{i in row u} alpha r_ui y_i y_i^T,   b_u = sum_{i in row u} (1 + alpha r_ui) y_i

and rounds x_u to fp32 once; an empty row gives zeros.  Pinned by tests/test_oracle_ials.py against a brute-force statement
over all cells that shares none of this algebra.
"""
import numpy as np


def normal_equations(row_ptr, col, val, Y, alpha, reg, G=None):
    """(A float64 [rows, d, d], b float64 [rows, d])"""
    Y = np.asarray(Y, dtype=np.float64)
    d = Y.shape[1]
    G = Y.T @ Y if G is None else np.asarray(G, dtype=np.float64)
    rows = len(row_ptr) - 1
    A = np.empty((rows, d, d))
    b = np.empty((rows, d))
    for u in range(rows):
        lo, hi = int(row_ptr[u]), int(row_ptr[u + 1])
        Yu = Y[np.asarray(col[lo:hi], dtype=np.int64)]
        w = float(alpha) * np.asarray(val[lo:hi], dtype=np.float64)
        A[u] = G + float(reg) * np.eye(d) + (Yu * w[:, None]).T @ Yu
        b[u] = ((1.0 + w)[:, None] * Yu).sum(0)
    return A, b


def half_sweep(row_ptr, col, val, Y, alpha, reg, round32=True):
    """X [rows, d]: float32 (the kernel's output format) or, round32=False, the float64 solutions"""
    A, b = normal_equations(row_ptr, col, val, Y, alpha, reg)
    X = np.zeros(b.shape)
    for u in range(len(b)):
        if row_ptr[u + 1] > row_ptr[u]:
            X[u] = np.linalg.solve(A[u], b[u])
    return X.astype(np.float32) if round32 else X


def objective(row_ptr, col, val, X, Y, alpha, reg):
    """sum over all cells of c (p - <x, y>)^2 + reg (|X|^2 + |Y|^2) by the Gram trick"""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    G = Y.T @ Y
    total = 0.0
    for u in range(len(row_ptr) - 1):
        lo, hi = int(row_ptr[u]), int(row_ptr[u + 1])
        s = Y[np.asarray(col[lo:hi], dtype=np.int64)] @ X[u]
        c = 1.0 + float(alpha) * np.asarray(val[lo:hi], dtype=np.float64)
        total += X[u] @ G @ X[u] + float((c * (1.0 - s) ** 2 - s ** 2).sum())
    return total + float(reg) * float((X ** 2).sum() + (Y ** 2).sum())


def transpose(row_ptr, col, val, n_cols):
    """the CSR of the transposed matrix, rows ascending within a column (what ops.slim_csr builds with swapped columns)"""
    rows = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    order = np.lexsort((rows, col))
    t_ptr = np.zeros(n_cols + 1, dtype=np.int64)
    t_ptr[1:] = np.cumsum(np.bincount(np.asarray(col, dtype=np.int64), minlength=n_cols))
    return t_ptr, rows[order].astype(np.int32), np.asarray(val)[order]


def fit(row_ptr, col, val, P0, Q0, alpha, reg, epochs, round32=True):
    """(P, Q, losses): `epochs` full sweeps - users, then items - from the tables (P0, Q0); round32: the tables are
    rounded to fp32 between half-sweeps (the kernels' path), else kept in fp64 throughout; the objective after each."""
    t_ptr, t_col, t_val = transpose(row_ptr, col, val, len(Q0))
    P, Q = np.asarray(P0, dtype=np.float64), np.asarray(Q0, dtype=np.float64)
    losses = []
    for _ in range(epochs):
        P = half_sweep(row_ptr, col, val, Q, alpha, reg, round32).astype(np.float64)
        Q = half_sweep(t_ptr, t_col, t_val, P, alpha, reg, round32).astype(np.float64)
        losses.append(objective(row_ptr, col, val, P, Q, alpha, reg))
    return P, Q, losses


# ---- fixtures shared by the CPU and the GPU tests ----------------------------------------------------------------------
ROW_LENGTHS = (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257)


def csr_of_lengths(lengths, n_cols, rng, ratings=(1, 6)):
    """a CSR whose row u has lengths[u] distinct ascending columns below n_cols and integer ratings in [1, 5]"""
    row_ptr = np.zeros(len(lengths) + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum(lengths)
    col = np.concatenate([np.sort(rng.choice(n_cols, n, replace=False)) for n in lengths] + [np.zeros(0, dtype=np.int64)])
    val = rng.integers(ratings[0], ratings[1], len(col)).astype(np.float32)
    return row_ptr, col.astype(np.int32), val


def exact_solve_fixture(d, seed, two_share=0.5):
    """L lower triangular, diagonal in {1, 2}, at most two entries +-1 per row within three columns of the diagonal;
    the item table is L^T (I = d), so that Y^T Y = L L^T exactly."""
    rng = np.random.default_rng(seed)
    L = np.diag(np.where(rng.random(d) < two_share, 2.0, 1.0))
    for i in range(1, d):
        cand = np.arange(max(0, i - 3), i)
        for j in rng.choice(cand, min(len(cand), int(rng.integers(0, 3))), replace=False):
            L[i, j] = float(rng.choice([-1.0, 1.0]))
    return L


def exact_solution(L, subset):
    """x = L^-T 1_S in exact rational arithmetic -> (list of Fractions, True when every element and every partial sum of
    the back substitution is exact in fp64 and the result is exact in fp32)"""
    from fractions import Fraction
    d = len(L)
    z = [Fraction(1 if i in subset else 0) for i in range(d)]
    x = [Fraction(0)] * d
    for i in range(d - 1, -1, -1):
        x[i] = (z[i] - sum(Fraction(int(L[j, i])) * x[j] for j in range(i + 1, d))) / int(L[i, i])
    ok = True
    for v in x:
        if v != 0:
            den, num = v.denominator, abs(v.numerator)
            ok &= den & (den - 1) == 0                                    # dyadic
            ok &= num.bit_length() - (num & -num).bit_length() + 1 <= 24  # fits an fp32 significand
            ok &= Fraction(1, 1 << 100) < abs(v) < (1 << 100)             # far inside fp32's exponent range
    # every partial sum is a multiple of 1 / (the largest denominator) and at most 1 + d max|x|: exact in fp64 if that
    # many grid steps fit 53 bits
    grid = max(v.denominator for v in x)
    ok &= (1 + d * max(abs(v) for v in x)) * grid < (1 << 53)
    return x, bool(ok)
