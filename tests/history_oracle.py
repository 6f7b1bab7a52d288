"""Numpy restatement of `get_history_matrix` (daisy/utils/utils.py:87-123), of the dense rows
`AERecommender.get_user_rating_matrix` builds from its padded pair (AbstractRecommender.py:147-158), of `AEDataset`'s
first-seen order and of `get_inter_matrix`'s COO columns, plus the FIXTURES the golden file, the host tests and the GPU
tests share.  Fixtures are rebuilt from their seeds; tests/golden/make_golden_history.py asserts that this
oracle equals the real reference on every fixture before it writes tests/golden/kat_history.npz.

  padded pair   a count per row; a stable argsort by row puts every row's entries side by side in frame order; the place
                of an entry inside its row is its rank in that run.  Values are float64 until the final cast to float32.
  dense rows    the padded pair written position by position, left to right: a later write of a column replaces an
                earlier one, and the padding (column 0, value 0) after a short row is a write like any other.
  CSR           two routes that must agree: the nonzeros of the dense rows, ascending; and the four rules applied to the
                frame directly (last of a duplicated pair, column 0 of a short row lost, column 0 of a longest row kept,
                float32 zeros dropped).
"""
import hashlib

import numpy as np

ROW_NUM, COL_NUM = 70, 130          # the `edges` fixture
LONGEST = 257

# the rows of `edges` that show one rule each (tests/test_oracle_history.py)
ROW_LAST_WINS = 0           # longest; (0, 7) appears three times with values 2, 0, 4 -> 4 stays
ROW_SHORT_LOSES_0 = 3       # 63 entries, holds column 0 with value 5 -> gone
ROW_TIED_KEEPS_0 = 6        # the second row of length 257, holds column 0 with value 3 -> stays (as does row 0's)
ROW_ZERO_DROPPED = 4        # 64 entries; column 9's last value is 0.0, column 11's is 1e-50 (0 in float32) -> both gone
ROW_ONLY_0 = 2              # one entry, column 0 -> an empty row
INEXACT = 0.1               # not representable in float32


# ---- the reference's functions, restated ---------------------------------------------------------------------------------
def history_matrix(row_ids, col_ids, values, row_num):
    """-> (ids int64 [R, L], vals float32 [R, L], lens int64 [R]); values None: all ones"""
    row_ids = np.asarray(row_ids, dtype=np.int64)
    col_ids = np.asarray(col_ids, dtype=np.int64)
    n = len(row_ids)
    values = np.ones(n) if values is None else np.asarray(values, dtype=np.float64)
    lens = np.bincount(row_ids, minlength=row_num).astype(np.int64)
    L = int(lens.max()) if row_num else 0
    ids = np.zeros((row_num, L), dtype=np.int64)
    vals = np.zeros((row_num, L), dtype=np.float64)
    if n:
        order = np.argsort(row_ids, kind="stable")
        begin = np.cumsum(lens) - lens
        place = np.arange(n) - begin[row_ids[order]]
        ids[row_ids[order], place] = col_ids[order]
        vals[row_ids[order], place] = values[order]
    return ids, vals.astype(np.float32), lens


def dense_rows(ids, vals, width):
    """[R, width] float32: every row's padded history written position by position (no accumulation)"""
    R, L = ids.shape
    out = np.zeros((R, width), dtype=np.float32)
    rows = np.arange(R)
    for p in range(L):
        out[rows, ids[:, p]] = vals[:, p]
    return out


def csr_of_dense(dense):
    """the nonzeros of every row, columns ascending -> (row_ptr int64, col int32, val float32)"""
    r, c = np.nonzero(dense)
    row_ptr = np.zeros(dense.shape[0] + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum(np.bincount(r, minlength=dense.shape[0]))
    return row_ptr, c.astype(np.int32), dense[r, c].astype(np.float32)


def csr_direct(row_ids, col_ids, values, row_num, col_num):
    """the same CSR from the frame and the four rules, never forming the padded pair -> (row_ptr, col, val, L)"""
    row_ids = np.asarray(row_ids, dtype=np.int64)
    col_ids = np.asarray(col_ids, dtype=np.int64)
    n = len(row_ids)
    v32 = (np.ones(n) if values is None else np.asarray(values, dtype=np.float64)).astype(np.float32)
    lens = np.bincount(row_ids, minlength=row_num)
    L = int(lens.max()) if row_num else 0
    key = row_ids * col_num + col_ids
    order = np.argsort(key, kind="stable")
    ks = key[order]
    tail = np.ones(n, dtype=bool)
    tail[:-1] = ks[1:] != ks[:-1]                                     # rule 1: the last of a duplicated pair
    r, c, v = row_ids[order], col_ids[order], v32[order]
    keep = tail & ~((c == 0) & (lens[r] < L)) & (v != 0)              # rules 2 / 3: column 0 and the padding; rule 4: zeros
    row_ptr = np.zeros(row_num + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum(np.bincount(r[keep], minlength=row_num))
    return row_ptr, c[keep].astype(np.int32), v[keep], L


def first_seen(ids):
    """the distinct values in order of first appearance, int64 (pandas.unique)"""
    ids = np.asarray(ids, dtype=np.int64)
    vals, where = np.unique(ids, return_index=True)
    return vals[np.argsort(where, kind="stable")]


def coo_columns(fx):
    return fx["user"].astype(np.int32), fx["item"].astype(np.int32), fx["rating"].astype(np.float64)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- fixtures ------------------------------------------------------------------------------------------------------------
def _frame(rows, cols, vals, row_num, col_num, rows_are):
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.float64)
    if rows_are == "user":
        return {"user": rows, "item": cols, "rating": vals, "user_num": row_num, "item_num": col_num}
    return {"user": cols, "item": rows, "rating": vals, "user_num": col_num, "item_num": row_num}


def _tiny():
    return _frame([3, 0, 3, 1, 0, 3, 1], [0, 0, 2, 0, 1, 0, 3], [5, 4, 0, 2, 3, 1, 2.5], 5, 4, "user")


def _edges_entries():
    """(row, col, val) row-contiguous.  Lengths 0, 1, 63, 64, 65 and 257 (wave and workgroup edges; 257 > 130 columns
    forces duplicates); absent rows; two rows tied for longest, both with column 0; short rows with column 0; duplicates
    with different values; exact zeros; one value float32 cannot hold and one it rounds to zero."""
    rng = np.random.default_rng(2301)
    lengths = [LONGEST, 0, 1, 63, 64, 65, LONGEST] + [(0, 1, 2, 3, 63, 64, 65, 7, 0, 1)[k % 10] for k in range(ROW_NUM - 7)]
    R, Cc, V = [], [], []
    for r, ln in enumerate(lengths):
        c = rng.integers(1, COL_NUM, ln)
        v = rng.integers(1, 6, ln).astype(np.float64)
        v[rng.random(ln) < 0.08] = 0.0
        if ln >= 2 and r % 3 == 0:
            c[ln // 2] = 0                                # column 0 somewhere in the middle of every third row
        if r == ROW_LAST_WINS:
            c[c == 7] = 8
            c[[5, 100, 200]], v[[5, 100, 200]] = 7, (2.0, 0.0, 4.0)
            c[30], v[30] = 0, 2.0
            c[250], v[250] = 0, 3.5                       # its column 0: written twice, the later value stays
        if r == ROW_ONLY_0:
            c[0], v[0] = 0, 4.0
        if r == ROW_SHORT_LOSES_0:
            c[c == 0] = 1
            c[10], v[10] = 0, 5.0
        if r == ROW_ZERO_DROPPED:
            c[c == 9], c[c == 11], c[c == 13] = 10, 12, 14
            c[[3, 40]], v[[3, 40]] = 9, (2.0, 0.0)        # nonzero first, zero last -> dropped
            c[50], v[50] = 11, 1e-50                      # a float64 that is 0 in float32 -> dropped
            c[[4, 41]], v[[4, 41]] = 13, (0.0, INEXACT)   # zero first, 0.1 last -> kept, rounded once
        if r == ROW_TIED_KEEPS_0:
            c[c == 0] = 1
            c[128], v[128] = 0, 3.0
        R.append(np.full(ln, r)), Cc.append(c), V.append(v)
    return np.concatenate(R), np.concatenate(Cc), np.concatenate(V)


def _edges(mixed, rows_are):
    r, c, v = _edges_entries()
    if mixed:                                             # the frame randomly interleaved (the order inside a row stays)
        labels = np.random.default_rng(2302).permutation(r)
        dest = np.argsort(labels, kind="stable")          # the k-th place that holds row x takes row x's k-th entry
        c2, v2 = np.empty_like(c), np.empty_like(v)
        c2[dest], v2[dest] = c, v
        r, c, v = labels, c2, v2
    return _frame(r, c, v, ROW_NUM, COL_NUM, rows_are)


CROSS_N = 262144 + 1000             # past the size at which the sort wrappers change algorithm


def _cross():
    rng = np.random.default_rng(2303)
    U, I, n = 3000, 2000, CROSS_N
    users = (rng.zipf(1.4, n) - 1) % U
    users[rng.permutation(n)[:n // 5]] = 17               # one row holds a fifth of the frame
    items = rng.integers(0, I, n)
    vals = rng.integers(0, 6, n).astype(np.float64)       # a sixth of the values is 0
    return _frame(users, items, vals, U, I, "user")


def _one_row():
    return _frame([1], [2], [2.0], 3, 4, "user")


def _row_num_1():
    return _frame([0, 0, 0, 0, 0, 0], [3, 0, 3, 1, 0, 4], [1, 2, 0, 3, 4, 0.1], 1, 5, "user")


def _empty():
    return _frame([], [], [], 3, 4, "user")


_BUILDERS = {"tiny": _tiny, "edges_mixed_u": lambda: _edges(True, "user"), "edges_mixed_i": lambda: _edges(True, "item"),
             "edges_contig_u": lambda: _edges(False, "user"), "edges_contig_i": lambda: _edges(False, "item"),
             "cross": _cross, "one_row": _one_row, "row_num_1": _row_num_1, "empty": _empty}
LARGE = ("cross",)                  # stored as history_len + SHA-256 of every array's bytes

# (fixture, row, use_config_value_name)
CASES = [("tiny", "user", True), ("tiny", "user", False), ("tiny", "item", True),
         ("edges_mixed_u", "user", True), ("edges_mixed_u", "user", False),
         ("edges_mixed_i", "item", True), ("edges_mixed_i", "item", False),
         ("edges_contig_u", "user", True), ("edges_contig_u", "user", False),
         ("edges_contig_i", "item", True), ("edges_contig_i", "item", False),
         ("cross", "user", True), ("cross", "user", False),
         ("one_row", "user", True), ("row_num_1", "user", True), ("row_num_1", "item", True),
         ("empty", "user", True), ("empty", "item", False)]

_cache = {}


def fixture(name):
    """the frame of a fixture (built once, shared, never written to)"""
    if name not in _cache:
        fx = _BUILDERS[name]()
        for k in ("user", "item", "rating"):
            fx[k].setflags(write=False)
        _cache[name] = fx
    return _cache[name]


def case_id(name, row, use_value):
    return f"{name}_{row}_{int(use_value)}"


def columns(fx, row, use_value):
    """(row_ids, col_ids, values or None, row_num, col_num) as get_history_matrix chooses them"""
    values = fx["rating"] if use_value else None
    if row == "user":
        return fx["user"], fx["item"], values, fx["user_num"], fx["item_num"]
    return fx["item"], fx["user"], values, fx["item_num"], fx["user_num"]


_results = {}


def expected(name, row, use_value):
    """the oracle's answers for a case, computed once: ids, vals, lens, csr (row_ptr, col, val, L)"""
    key = case_id(name, row, use_value)
    if key not in _results:
        r, c, v, R, Cn = columns(fixture(name), row, use_value)
        ids, vals, lens = history_matrix(r, c, v, R)
        _results[key] = {"ids": ids, "vals": vals, "lens": lens, "csr": csr_direct(r, c, v, R, Cn)}
    return _results[key]
