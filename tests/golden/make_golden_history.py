#!/usr/bin/env python
"""Golden values for get_history_matrix, AEDataset and get_inter_matrix, generated from the REAL reference
(`daisy.utils.utils` and `daisy.utils.dataset`, imported from the reference checkout; nothing is copied).  Runs only where
the reference exists; the output is committed:

    python tests/golden/make_golden_history.py            # -> tests/golden/kat_history.npz
    python tests/golden/make_golden_history.py --time     # only prints the reference's seconds per 200 000 rows on this host

Per case of tests/history_oracle.py::CASES (`<fixture>_<row>_<values>_*`; the frames are rebuilt from the fixture's seed):
the reference's history_matrix, history_value and history_len.  Per fixture: AEDataset's `.data` for the user and the
item column, and the row / col / data of get_inter_matrix's COO.  The fixtures named in LARGE are stored as history_len
plus the SHA-256 of every array's bytes - every comparison is exact, so a digest loses nothing.

Before anything is written the script ASSERTS that the oracle equals all of it: if that fails the oracle is wrong - do
not change a seed.
"""
import logging
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402,F401  (puts the reference checkout and the logging shims on sys.path)

import pandas as pd  # noqa: E402

from daisy.utils.dataset import AEDataset  # noqa: E402
from daisy.utils.utils import get_history_matrix, get_inter_matrix  # noqa: E402

import history_oracle as O  # noqa: E402

warnings.filterwarnings("ignore")


def config(fx):
    return {"UID_NAME": "user", "IID_NAME": "item", "INTER_NAME": "rating", "user_num": fx["user_num"],
            "item_num": fx["item_num"], "logger": logging.getLogger("golden")}


def frame_of(fx):
    return pd.DataFrame({"user": fx["user"], "item": fx["item"], "rating": fx["rating"]})


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def time_reference():
    rng = np.random.default_rng(0)
    n = 200_000
    fx = {"user": rng.integers(0, 6000, n), "item": rng.integers(0, 4000, n), "rating": np.ones(n), "user_num": 6000,
          "item_num": 4000}
    t0 = time.perf_counter()
    get_history_matrix(frame_of(fx), config(fx), row="user")
    print(f"reference get_history_matrix, {n} rows, 6000 users: {time.perf_counter() - t0:.2f} s")


def main():
    if "--time" in sys.argv:
        return time_reference()
    out = {}
    for name, row, use_value in O.CASES:
        fx = O.fixture(name)
        ids, vals, lens = get_history_matrix(frame_of(fx), config(fx), row=row, use_config_value_name=use_value)
        ids, vals, lens = ids.numpy(), vals.numpy(), lens.numpy()
        mine = O.expected(name, row, use_value)
        tag = O.case_id(name, row, use_value)
        assert same(mine["ids"], ids) and same(mine["vals"], vals) and same(mine["lens"], lens), tag
        out[f"{tag}_len"] = lens
        if name in O.LARGE:
            out[f"{tag}_ids_sha"], out[f"{tag}_vals_sha"] = np.array(O.digest(ids)), np.array(O.digest(vals))
            out[f"{tag}_shape"] = np.array(ids.shape, dtype=np.int64)
        else:
            out[f"{tag}_ids"], out[f"{tag}_vals"] = ids, vals
        print(f"{tag}: {len(fx['user'])} rows -> {ids.shape}: oracle == reference")
    for name in O._BUILDERS:
        fx, df = O.fixture(name), frame_of(O.fixture(name))
        for col in ("user", "item"):
            ref = np.asarray(AEDataset(df, yield_col=col).data)
            assert same(O.first_seen(fx[col]), ref.astype(np.int64)), (name, col)
            out[f"{name}_first_{col}"] = ref.astype(np.int64)
        m = get_inter_matrix(df, config(fx), "coo")
        r, c, d = O.coo_columns(fx)
        assert same(r, m.row) and same(c, m.col) and same(d, m.data) and m.shape == (fx["user_num"], fx["item_num"]), name
        if name in O.LARGE:
            for k, a in (("row", m.row), ("col", m.col), ("data", m.data)):
                out[f"{name}_coo_{k}_sha"] = np.array(O.digest(a))
        else:
            out[f"{name}_coo_row"], out[f"{name}_coo_col"], out[f"{name}_coo_data"] = m.row, m.col, m.data
        print(f"{name}: AEDataset and the COO columns: oracle == reference")
    # the values the issue text quotes for `tiny`
    assert out["tiny_user_1_ids"].tolist() == [[0, 1, 0], [0, 3, 0], [0, 0, 0], [0, 2, 0], [0, 0, 0]]
    assert out["tiny_user_1_vals"].tolist() == [[4, 3, 0], [2, 2.5, 0], [0, 0, 0], [5, 0, 1], [0, 0, 0]]
    assert out["tiny_user_1_len"].tolist() == [2, 2, 0, 3, 0] and out["tiny_first_user"].tolist() == [3, 0, 1]
    path = os.path.join(HERE, "kat_history.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
