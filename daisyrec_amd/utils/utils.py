"""Device-side replacements for the two host loops of daisy/utils/utils.py that sit either side
of the MF hot path at scale:

* ``get_ur``               utils.py:19-34  (Python iterrows loop)       -> ``user_csr`` (device CSR), and ``get_ur`` /
                                                                          ``get_ir`` with the reference's return type
                                                                          (dict of sets) built without the row loop
* ``build_candidates_set`` utils.py:53-85  (O(U*I) np.setdiff1d loop)   -> same name, same return
"""
from __future__ import annotations

from collections import defaultdict

import numpy as np
import torch

from .. import ops


def _grouped_sets(keys, vals):
    out = defaultdict(set)
    keys, vals = np.asarray(keys).astype(np.int64), np.asarray(vals).astype(np.int64)
    if keys.size == 0:
        return out
    order = np.argsort(keys, kind="stable")
    ks, vs = keys[order], vals[order]
    cuts = np.flatnonzero(ks[1:] != ks[:-1]) + 1
    for k, chunk in zip(ks[np.r_[0, cuts]].tolist(), np.split(vs, cuts)):
        out[k] = set(chunk.tolist())
    return out


def get_ur(df):
    """utils.py:19-34: {user: set(items)} as a defaultdict(set) with int keys - the same object the reference's
    row loop builds (1.9 s per 100 k rows there), from one sort (host numpy: this dict is host data by contract)."""
    return _grouped_sets(df["user"].to_numpy(), df["item"].to_numpy())


def get_ir(df):
    """utils.py:36-51: {item: set(users)}"""
    return _grouped_sets(df["item"].to_numpy(), df["user"].to_numpy())


def user_csr(df_or_pairs, user_num, device="cuda"):
    """(indptr int64[U+1], sorted items int32[n]) of the (user, item) pairs of a DataFrame
    (columns 'user', 'item') or of a (users, items) pair of arrays."""
    if hasattr(df_or_pairs, "columns"):
        users, items = df_or_pairs["user"].to_numpy(), df_or_pairs["item"].to_numpy()
    else:
        users, items = df_or_pairs
    users = torch.as_tensor(np.asarray(users).astype(np.int32)).to(device)
    items = torch.as_tensor(np.asarray(items).astype(np.int32)).to(device)
    return ops.build_user_csr(users, items, user_num)


def _ur_pairs(ur):
    us = np.fromiter((u for u, s in ur.items() for _ in s), dtype=np.int32)
    it = np.fromiter((i for _, s in ur.items() for i in s), dtype=np.int32)
    return us, it


def build_candidates_set(test_ur, train_ur, config, drop_past_inter=True):
    """Same signature and return value as utils.py:53-85: (test_u, test_ucands) with
    test_ucands = [[u, np.ndarray(cand_num)], ...] in test_ur's key order.  Negatives come from the
    device generator (Philox keyed by config['seed']); truths are appended in ascending order."""
    if not drop_past_inter:
        raise NotImplementedError("drop_past_inter=False is not used by the drivers (test.py:112, tune.py:204)")
    if not torch.cuda.is_available():
        raise RuntimeError("daisyrec_amd.build_candidates_set needs a HIP device (no CPU fallback)")
    user_num, item_num, cand_num = config["user_num"], config["item_num"], config["cand_num"]
    dev = config.get("device", "cuda")
    ip_te, it_te = user_csr(_ur_pairs(test_ur), user_num, dev)
    ip_tr, it_tr = user_csr(_ur_pairs(train_ur), user_num, dev)
    test_u = list(test_ur.keys())
    users = torch.as_tensor(np.asarray(test_u, dtype=np.int64)).to(dev)
    cands = ops.build_candidates(ip_te, it_te, ip_tr, it_tr, users, item_num, cand_num,
                                 int(config.get("seed", 2022))).cpu().numpy()
    return test_u, [[u, cands[k]] for k, u in enumerate(test_u)]


# ---- get_history_matrix / get_inter_matrix (utils.py:87-144) ----------------------------------------------
def _check_codes(ids, num, what):
    """IndexError for an id outside [0, num), on the host and before any launch.  (The reference indexes numpy arrays
    with them: too large an id raises there as well, a negative one wraps - refused here)"""
    if ids.size:
        lo, hi = int(ids.min()), int(ids.max())
        if lo < 0 or hi >= int(num):
            bad = hi if hi >= int(num) else lo
            raise IndexError(f"index {bad} is out of bounds for axis 0 with size {int(num)} ({what} ids must lie in "
                             f"[0, {int(num)}))")


def _history_columns(df, config, row, use_config_value_name, what):
    """The part of get_history_matrix before its loops (utils.py:91-105): the assertion, the row / column choice and
    the value column; then the range check and the device columns (int32 codes, float64 values or None for ones)."""
    assert row in df.columns, f'invalid name {row}: not in columns of history dataframe'
    uid_name, iid_name = config['UID_NAME'], config['IID_NAME']
    user_ids, item_ids = df[uid_name].values, df[iid_name].values
    value_name = config['INTER_NAME'] if use_config_value_name else None
    user_num, item_num = config['user_num'], config['item_num']
    if row == 'user':
        row_num, max_col_num = user_num, item_num
        row_ids, col_ids = user_ids, item_ids
    else:  # 'item'
        row_num, max_col_num = item_num, user_num
        row_ids, col_ids = item_ids, user_ids
    row_ids, col_ids = np.asarray(row_ids), np.asarray(col_ids)
    _check_codes(row_ids, row_num, row)
    _check_codes(col_ids, max_col_num, "column")
    if not torch.cuda.is_available():
        raise RuntimeError(f"daisyrec_amd.{what} needs a HIP device (no CPU fallback)")
    dev = torch.device(config.get("device", "cuda"))
    cols = None
    if len(row_ids):
        r = torch.from_numpy(np.ascontiguousarray(row_ids, dtype=np.int32)).to(dev)
        c = torch.from_numpy(np.ascontiguousarray(col_ids, dtype=np.int32)).to(dev)
        # values: float64 on the host (np.ones / the frame's column stored into a float64 matrix, utils.py:98,116), cast
        # to float32 once on the device (torch.FloatTensor, utils.py:123)
        v = None if value_name is None else torch.from_numpy(
            np.ascontiguousarray(df[value_name].values, dtype=np.float64)).to(dev)
        cols = (r, c, v)
    return cols, int(row_num), int(max_col_num), dev


def get_history_matrix(df, config, row='user', use_config_value_name=False):
    """utils.py:87-123 without its two loops over the rows: (history_matrix int64 [R, L], history_value float32 [R, L],
    history_len int64 [R]) as DEVICE tensors, cell for cell the reference's.  One stable sort by row code gives the order
    inside a row; one kernel writes every cell once.  The padded pair costs R * L * 12 bytes: when that does not fit the
    device's free memory a MemoryError says so - history_csr gives VAECF the same rows from the interactions alone."""
    logger = config['logger']
    cols, row_num, max_col_num, dev = _history_columns(df, config, row, use_config_value_name, "get_history_matrix")
    if cols is None:
        return (torch.zeros((row_num, 0), dtype=torch.int64, device=dev), torch.zeros((row_num, 0), dtype=torch.float32, device=dev),
                torch.zeros(row_num, dtype=torch.int64, device=dev))
    r, c, v = cols
    history_len, col_num, order, start = ops.history_counts(r, row_num, validate=False)
    if col_num > max_col_num * 0.2:
        logger.info(f'Max value of {row}\'s history interaction records has reached: {col_num / max_col_num * 100:.4f}% of the total.')
    need = row_num * col_num * 12
    free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    if need > free:
        raise MemoryError(f"get_history_matrix: the padded [{row_num}, {col_num}] pair needs {need} bytes, the device has "
                          f"{free} free; use daisyrec_amd.utils.utils.history_csr (config['history_csr']), which is "
                          "bounded by the interactions")
    history_matrix, history_value = ops.history_fill(order, start, c, v, row_num, col_num)
    return history_matrix, history_value, history_len


def history_csr(df, config, row='user', use_config_value_name=False):
    """The rows get_history_matrix's pair stands for under AERecommender.get_user_rating_matrix, as a device CSR and
    without the padded pair: (row_ptr int64 [R + 1], col int32 [nnz], val float32 [nnz], L).  Byte for byte
    ops.vae_history_csr of get_history_matrix's tensors; config['history_csr'] hands it to VAECF."""
    cols, row_num, max_col_num, dev = _history_columns(df, config, row, use_config_value_name, "history_csr")
    if cols is None:
        return (torch.zeros(row_num + 1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                torch.zeros(0, dtype=torch.float32, device=dev), 0)
    r, c, v = cols
    return ops.history_csr(r, c, v, row_num, max_col_num, validate=False)


class DeviceInterMatrix:
    """What get_inter_matrix returns here: the interaction frame as device columns, with the corner of scipy's COO
    interface the recommenders read.  row / col int32 and data float64, in frame order, duplicates kept - as
    sp.coo_matrix((data, (src, tar))) keeps them."""
    format = "coo"

    def __init__(self, row, col, data, shape):
        self.row, self.col, self.data = row, col, data
        self.shape = (int(shape[0]), int(shape[1]))

    @property
    def nnz(self):
        return int(self.row.numel())

    def tocoo(self):
        return self

    def to_scipy(self):
        import scipy.sparse as sp
        return sp.coo_matrix((self.data.cpu().numpy(), (self.row.cpu().numpy(), self.col.cpu().numpy())), shape=self.shape)


def get_inter_matrix(df, config, form='coo'):
    """utils.py:125-144: the whole interaction matrix.  'coo': a DeviceInterMatrix (LightGCN / NGCF hand its columns to
    the graph builder: no scipy build, one host-to-device copy); 'csr': the scipy CSR of the same frame."""
    value_field = config['INTER_NAME']
    src_field, tar_field = config['UID_NAME'], config['IID_NAME']
    user_num, item_num = config['user_num'], config['item_num']
    if form not in ('coo', 'csr'):
        raise NotImplementedError(f'Sparse matrix format [{form}] has not been implemented...')
    src, tar = np.asarray(df[src_field].values), np.asarray(df[tar_field].values)
    data = np.asarray(df[value_field].values)
    _check_codes(src, user_num, "user")
    _check_codes(tar, item_num, "item")
    if not torch.cuda.is_available():
        raise RuntimeError("daisyrec_amd.get_inter_matrix needs a HIP device (no CPU fallback)")
    dev = torch.device(config.get("device", "cuda"))
    mat = DeviceInterMatrix(torch.from_numpy(np.ascontiguousarray(src, dtype=np.int32)).to(dev),
                            torch.from_numpy(np.ascontiguousarray(tar, dtype=np.int32)).to(dev),
                            torch.from_numpy(np.ascontiguousarray(data, dtype=np.float64)).to(dev), (user_num, item_num))
    return mat if form == 'coo' else mat.to_scipy().tocsr()
