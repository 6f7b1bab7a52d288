"""Mirror of `daisy.utils.loader.Preprocessor` (loader.py:144-320) on the HIP path: `process(df)` runs dedup, the rating
threshold, the N-filter / N-core, the category encoding, the sort by time and `item_pop` in one library call
(`daisy_prep_process`, csrc/prep.hip) instead of Python loops over rows per peel round.  `RawDataReader` is file parsing and
stays the reference's.  Constructor keys and attributes are the reference's: `user_num`, `item_num`, `item_pop`,
`uid_token`, `iid_token`, `token_uid`, `token_iid`, `get_user_num()`, `get_item_num()`; `rounds` (the peel rounds of the last
`Ncore` / `ui` call that removed rows) is ours.

`process` returns a new frame: the input's columns in their order (further columns are carried by `df.iloc[rows]`), a fresh
`RangeIndex`, `user` / `item` in the dtype `pd.Categorical(...).codes` gives, `rating` = 1.0 under `binary_inter`.  Id
columns that are not integers (strings) are factorised on the host (`pd.factorize(sort=True)`); the device sees integers.
Timestamps may be any integer dtype or datetime64 (taken as its int64 view).

Deviations from the reference:
  * timestamp ties: `sort_values` there is an unstable quicksort; ours is stable, tied rows stay in input order.  Frames
    with distinct timestamps come out identical.
  * an empty result (an empty core) is an empty frame with `user_num == item_num == 0`.
There is no CPU path: without a HIP device `process` raises.
"""
from __future__ import annotations

import re

import numpy as np
import pandas as pd
import torch

from .. import ops


def _codes_dtype(n_categories):
    """the dtype of pd.Categorical(...).codes for that many categories"""
    for dt in (np.int8, np.int16, np.int32):
        if n_categories < np.iinfo(dt).max:       # pandas' coerce_indexer_dtype: 127 categories are already int16
            return dt
    return np.int64


def int64_column(col, what):
    """a timestamp column as int64: any integer dtype, or datetime64 by its int64 view; TypeError otherwise"""
    arr = col.to_numpy() if hasattr(col, "to_numpy") else np.asarray(col)
    if arr.dtype.kind in "iu":
        if arr.dtype == np.uint64 and arr.size and arr.max() > np.iinfo(np.int64).max:
            raise TypeError(f"{what}: uint64 values above int64's range")
        return np.ascontiguousarray(arr, dtype=np.int64)
    if arr.dtype.kind == "M":
        return np.ascontiguousarray(arr.view(np.int64))
    raise TypeError(f"{what}: dtype {col.dtype} is neither an integer nor datetime64")


def id_column(col):
    """-> (int64 ids for the device, host tokens or None): integers go as they are; anything else is factorised on the
    host in sorted order, so the device's ranks are the reference's category codes"""
    arr = col.to_numpy()
    if arr.dtype.kind in "iu" and not (arr.dtype == np.uint64 and arr.size and arr.max() > np.iinfo(np.int64).max):
        return np.ascontiguousarray(arr, dtype=np.int64), None
    codes, uniques = pd.factorize(arr, sort=True)
    if (codes < 0).any():
        raise ValueError("an id column holds missing values")
    return codes.astype(np.int64), np.asarray(uniques)


def parse_prepro(prepro, level):
    """-> (mode, N) of 'origin' / 'Nfilter' / 'Ncore'; the reference's ValueErrors (loader.py:254, 299, 304)"""
    if prepro == "origin":
        return "origin", 1
    if isinstance(prepro, str) and (prepro.endswith("filter") or prepro.endswith("core")):
        nums = re.findall(r"\d+", prepro)
        if nums:
            if level not in ops.PREP_LEVELS:
                raise ValueError(f"Invalid level value: {level}")
            N = int(nums[0])
            if N < 1:
                raise ValueError(f"Invalid dataset preprocess type {prepro!r}: N must be >= 1")
            return ("filter" if prepro.endswith("filter") else "core"), N
    raise ValueError("Invalid dataset preprocess type, origin/Ncore/Nfilter (N is int number) expected")


class Preprocessor(object):
    def __init__(self, config):
        self.src = config['dataset']
        self.prepro = config['prepro']
        self.uid_name = config['UID_NAME']
        self.iid_name = config['IID_NAME']
        self.tid_name = config['TID_NAME']
        self.inter_name = config['INTER_NAME']
        self.binary = config['binary_inter']
        self.pos_threshold = config['positive_threshold']
        self.level = config['level']  # ui, u, i
        self.logger = config['logger']
        self.device = config.get('device', 'cuda') if hasattr(config, 'get') else 'cuda'

        self.get_pop = True if 'popularity' in config['metrics'] else False

        self.user_num, self.item_num = None, None
        self.item_pop = None
        self.rounds = 0

    def get_user_num(self):
        return self.user_num

    def get_item_num(self):
        return self.item_num

    def process(self, df):
        mode, N = parse_prepro(self.prepro, self.level)
        ts = int64_column(df[self.tid_name], f"column {self.tid_name!r}")
        thr = self.pos_threshold
        rating = None
        if thr is not None:
            rating = np.ascontiguousarray(df[self.inter_name].to_numpy(), dtype=np.float64)
            thr = float(thr)
        users, utok_host = id_column(df[self.uid_name])
        items, itok_host = id_column(df[self.iid_name])
        if not torch.cuda.is_available():
            raise RuntimeError("daisyrec_amd.Preprocessor.process needs a HIP device (no CPU fallback)")
        n = len(df)
        if n == 0:
            res = {"rows": np.zeros(0, np.int64), "user": np.zeros(0, np.int32), "item": np.zeros(0, np.int32),
                   "uid_token": np.zeros(0, np.int64), "iid_token": np.zeros(0, np.int64), "item_pop": np.zeros(0),
                   "user_num": 0, "item_num": 0, "rounds": 0}
        else:
            dev = self.device
            out = ops.prep_process(torch.from_numpy(users).to(dev), torch.from_numpy(items).to(dev),
                                   None if rating is None else torch.from_numpy(rating).to(dev),
                                   torch.from_numpy(ts).to(dev), threshold=thr, mode=mode, level=self.level if mode != "origin"
                                   else "ui", N=N, want_pop=self.get_pop)
            res = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
        self.user_num, self.item_num, self.rounds = res["user_num"], res["item_num"], res["rounds"]
        uid_token, iid_token = res["uid_token"], res["iid_token"]
        self.uid_token = uid_token if utok_host is None else utok_host[uid_token]
        self.iid_token = iid_token if itok_host is None else itok_host[iid_token]
        if utok_host is None:
            self.uid_token = self.uid_token.astype(df[self.uid_name].to_numpy().dtype, copy=False)
        if itok_host is None:
            self.iid_token = self.iid_token.astype(df[self.iid_name].to_numpy().dtype, copy=False)
        self.token_uid = {uid: token for token, uid in enumerate(self.uid_token)}
        self.token_iid = {iid: token for token, iid in enumerate(self.iid_token)}

        new = df.iloc[res["rows"]].reset_index(drop=True)
        new[self.uid_name] = res["user"].astype(_codes_dtype(self.user_num))
        new[self.iid_name] = res["item"].astype(_codes_dtype(self.item_num))
        if self.binary:
            new[self.inter_name] = 1.0
        if self.get_pop:
            pop = res["item_pop"]
            self.item_pop = np.zeros(self.item_num) if pop is None else np.asarray(pop, dtype=np.float64)

        self.logger.info(f'Finish loading [{self.src}]-[{self.prepro}] dataset')
        return new
