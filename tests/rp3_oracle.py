"""numpy restatement of the two-hop walk with a per-row top-K (include/daisyrec_amd.h, daisy_walk2_topk) and
of the RP3beta / P3alpha model around it.  The walk repeats the kernel's contract operation by operation - every product
rounded to float32, added in float32 over the source row's entries in stored order, one rounded multiply by the column
scale, selection by (-w, j) - so the GPU tests compare by equality.  numpy's float32 arithmetic rounds every operation on
its own (there is no fused multiply-add to contract into)."""
import numpy as np

F32 = np.float32


def csr_of(dense):
    """(row_ptr int64, col int32 ascending, val float32) of the non-zero cells of a dense matrix"""
    dense = np.asarray(dense)
    rows, cols = np.nonzero(dense)
    ptr = np.zeros(dense.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=dense.shape[0]), out=ptr[1:])
    return ptr, cols.astype(np.int32), dense[rows, cols].astype(F32)


def csr_pattern(mask, row_values=None, values=None):
    """the CSR of a boolean pattern with the value row_values[row] (or values[row, col], or 1) on every stored cell"""
    rows, cols = np.nonzero(mask)
    ptr = np.zeros(mask.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=mask.shape[0]), out=ptr[1:])
    if row_values is not None:
        val = np.asarray(row_values)[rows]
    elif values is not None:
        val = np.asarray(values)[rows, cols]
    else:
        val = np.ones(len(rows))
    return ptr, cols.astype(np.int32), val.astype(F32)


def dense_of(csr, n_cols, dtype=np.float64):
    ptr, col, val = csr
    out = np.zeros((len(ptr) - 1, n_cols), dtype=dtype)
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    out[rows, col[:len(rows)]] = val[:len(rows)]
    return out


def walk_row(A, B, i, n_cols):
    """acc float32 [n_cols] of row i: sequential over the row's entries u in stored order"""
    a_ptr, a_col, a_val = A
    b_ptr, b_col, b_val = B
    acc = np.zeros(n_cols, dtype=F32)
    for e in range(a_ptr[i], a_ptr[i + 1]):
        u, a = a_col[e], F32(a_val[e])
        lo, hi = b_ptr[u], b_ptr[u + 1]
        js = b_col[lo:hi]                                   # distinct within a row: one add per cell
        acc[js] = acc[js] + a * b_val[lo:hi].astype(F32)    # float32 product, then float32 sum
    return acc


def select_row(w, K):
    """the columns of the K largest strictly positive weights, ties to the lower column, in ascending column order"""
    idx = np.flatnonzero(w > 0)                             # zero, negative and NaN are never kept
    order = np.lexsort((idx, -w[idx].astype(np.float64)))
    return np.sort(idx[order[:K]])


def walk2_topk(A, B, n_cols, K, col_scale=None, zero_diagonal=True, normalize=False):
    """-> (count int32 [n_rows], cols int32 [n_rows, K], vals float32 [n_rows, K]), unused slots (-1, 0)"""
    n_rows = len(A[0]) - 1
    count = np.zeros(n_rows, dtype=np.int32)
    cols = np.full((n_rows, K), -1, dtype=np.int32)
    vals = np.zeros((n_rows, K), dtype=F32)
    for i in range(n_rows):
        w = walk_row(A, B, i, n_cols)
        if col_scale is not None:
            w = w * np.asarray(col_scale, dtype=F32)
        if zero_diagonal and i < n_cols:
            w[i] = 0
        keep = select_row(w, K)
        v = w[keep].astype(F32)
        if normalize and len(keep):
            s = F32(0)
            for x in v:                                     # sequential, ascending column
                s = F32(s + x)
            v = (v / s).astype(F32)
        count[i] = len(keep)
        cols[i, :len(keep)] = keep
        vals[i, :len(keep)] = v
    return count, cols, vals


def dense_rows(count, cols, vals, n_cols, dtype=np.float64):
    """the fixed-pitch result as a dense [n_rows, n_cols] matrix"""
    out = np.zeros((len(count), n_cols), dtype=dtype)
    for i, c in enumerate(count):
        out[i, cols[i, :c]] = vals[i, :c]
    return out


# ---- the cases both test files use ------------------------------------------------------------------------------------
U, I, DENSITY = 300, 200, 0.08         # the shape of the exact case


def pattern(seed=0, users=U, items=I, density=DENSITY):
    return np.random.default_rng(seed).random((users, items)) < density


def dyadic_case(seed=0):
    """A[i, u] = s_i, B[u, j] = s_u on the stored cells, col_scale = s_i, s = 2^-floor(log2 deg): every product is a power
    of two and every sum of at most 300 of them over a span of a few binades is exact in float32"""
    X = pattern(seed)

    def dyadic(deg):
        out = np.zeros(len(deg))
        out[deg > 0] = 2.0 ** -np.floor(np.log2(deg[deg > 0]))
        return out

    s_user, s_item = dyadic(X.sum(1)), dyadic(X.sum(0))
    A = csr_pattern(X.T, row_values=s_item)
    B = csr_pattern(X, row_values=s_user)
    return X, A, B, s_item.astype(np.float32)


# ---- the model -------------------------------------------------------------------------------------------------------
def model_scales(X, alpha, beta):
    """(user_scale, item_scale, col_scale) float32 of a training matrix X [U, I] (dense, >= 0): (row sum)^-alpha,
    (column sum)^-alpha and (users of the item)^-beta in float64, rounded once; 0 where there is nothing"""
    X = np.asarray(X, dtype=np.float64)

    def neg_pow(t, p):
        out = np.zeros_like(t)
        out[t > 0] = t[t > 0] ** -p
        return out.astype(F32)

    return neg_pow(X.sum(1), alpha), neg_pow(X.sum(0), alpha), neg_pow((X != 0).sum(0).astype(np.float64), beta)


def model_operands(X, alpha):
    """(Piu, Pui) CSR triples: x^alpha * (row sum)^-alpha in float64, rounded once to float32"""
    X = np.asarray(X, dtype=np.float64)
    out = []
    for M in (X.T, X):
        tot = M.sum(1, keepdims=True)
        scale = np.zeros_like(tot)
        scale[tot > 0] = tot[tot > 0] ** -alpha
        out.append(csr_pattern(M != 0, values=(M ** alpha) * scale))
    return out[0], out[1]


def scores(X, W):
    """float64 [U, I] = X W with the terms of every cell added in ascending inner index (the products of two float32
    values are exact in float64): what daisy_knn_rank computes.  X [U, n] and W [n, I] dense."""
    X, W = np.asarray(X, dtype=np.float64), np.asarray(W, dtype=np.float64)
    S = np.zeros((X.shape[0], W.shape[1]))
    for i in range(X.shape[1]):
        us, js = np.flatnonzero(X[:, i]), np.flatnonzero(W[i])
        if len(us) and len(js):
            S[np.ix_(us, js)] += X[us, i][:, None] * W[i, js][None, :]
    return S


def top_ids(row, topk, cands=None):
    """the positions (candidate ids) of the topk largest scores, ties to the lower position"""
    order = np.lexsort((np.arange(len(row)), -row))[:topk]
    return order if cands is None else np.asarray(cands)[order]
