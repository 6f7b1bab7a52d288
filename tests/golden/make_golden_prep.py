#!/usr/bin/env python
"""Golden values for the Preprocessor and the splitters, generated from the REAL reference (`daisy.utils.loader.Preprocessor`
and `daisy.utils.splitter`, imported from the reference checkout; nothing is copied).  Runs only where the reference
exists; the output is committed:

    python tests/golden/make_golden_prep.py            # -> tests/golden/kat_prep.npz
    python tests/golden/make_golden_prep.py --time     # only prints the reference's seconds on this host

Per fixture of tests/prep_oracle.py::PREP_FIXTURES without `ties` (`<tag>_*`; the frames are rebuilt from the fixture's
seed): the surviving rows (an extra column holds the original row number), the codes with their dtypes, the tokens,
item_pop, user_num and item_num of the reference's `process`.  `empty_status` records what the reference does on a frame
whose core is empty.  Per SPLIT_FIXTURES frame: the reference's tloo ids, its utfo ids on the user-contiguous frames, the
per-user ufo counts and the rsbr / rloo sizes; tsbr ids and scikit-learn's unshuffled KFold for cv.

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
from sklearn.model_selection import KFold  # noqa: E402

from daisy.utils.loader import Preprocessor  # noqa: E402
from daisy.utils import splitter as RS  # noqa: E402

import prep_oracle as O  # noqa: E402

warnings.filterwarnings("ignore")


def config(fx):
    return {"dataset": "fixture", "prepro": fx["prepro"], "UID_NAME": "user", "IID_NAME": "item", "TID_NAME": "timestamp",
            "INTER_NAME": "rating", "binary_inter": True, "positive_threshold": fx.get("threshold"), "level": fx["level"],
            "logger": logging.getLogger("golden"), "metrics": ["popularity"]}


def frame_of(cols):
    df = pd.DataFrame({k: cols[k] for k in ("user", "item", "rating", "timestamp")})
    df["row"] = np.arange(len(df), dtype=np.int64)
    return df


def storable(tokens):
    tokens = np.asarray(tokens)
    return tokens.astype(str) if tokens.dtype == object else tokens


def reference_process(fx):
    p = Preprocessor(config(fx))
    out = p.process(frame_of(O.prep_frame(fx)))
    assert list(out.index) == list(range(len(out)))
    return {"rows": out["row"].to_numpy(), "user": out["user"].to_numpy(), "item": out["item"].to_numpy(),
            "uid_token": storable(p.uid_token), "iid_token": storable(p.iid_token), "item_pop": p.item_pop,
            "user_num": p.user_num, "item_num": p.item_num}, out


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and np.array_equal(a, b)


def per_user_counts(user, ids):
    ids = pd.Series(ids).dropna().to_numpy().astype(np.int64)
    tok = np.unique(user)
    return np.bincount(np.searchsorted(tok, user[ids]), minlength=len(tok))


def time_reference():
    rng = np.random.default_rng(0)
    n = 100_000
    df = pd.DataFrame({"user": rng.integers(0, 6000, n), "item": rng.zipf(1.3, n) % 4000, "rating": 1.0,
                       "timestamp": rng.permutation(n)})
    fx = dict(prepro="5core", level="ui")
    t0 = time.perf_counter()
    out = Preprocessor(config(fx)).process(df.copy())
    t1 = time.perf_counter()
    RS.split_test(out, "ufo", 0.2)
    t2 = time.perf_counter()
    print(f"reference Preprocessor.process, 5core / ui, {n} rows -> {len(out)}: {t1 - t0:.2f} s")
    print(f"reference split_test('ufo'), {len(out)} rows, {out['user'].nunique()} users: {t2 - t1:.2f} s")


def main():
    if "--time" in sys.argv:
        return time_reference()
    out = {}
    for tag, fx in O.PREP_FIXTURES.items():
        if fx.get("ties"):
            continue
        cols = O.prep_frame(fx)
        mine = O.process(cols["user"], cols["item"], cols["rating"], cols["timestamp"], fx["prepro"], fx["level"],
                         fx.get("threshold"))
        try:
            ref, frame = reference_process(fx)
        except Exception as e:          # noqa: BLE001  (what the reference does on an empty core is recorded, not judged)
            assert tag == "empty", (tag, e)
            out["empty_status"] = np.array(f"raises {type(e).__name__}")
            assert mine["user_num"] == 0 and len(mine["rows"]) == 0
            print(f"{tag}: the reference raises {type(e).__name__}: {e}")
            continue
        if tag == "empty":
            out["empty_status"] = np.array("returns an empty frame")
        for k in ("rows", "user", "item", "item_pop"):
            assert same(mine[k], ref[k]), (tag, k, mine[k][:8], ref[k][:8])
        for k in ("uid_token", "iid_token"):
            assert np.array_equal(storable(mine[k]), ref[k]), (tag, k)
        assert (mine["user_num"], mine["item_num"]) == (ref["user_num"], ref["item_num"]), tag
        assert (frame["rating"] == 1.0).all() and frame["rating"].dtype == np.float64
        for k in ("rows", "user", "item", "uid_token", "iid_token", "item_pop"):
            out[f"{tag}_{k}"] = ref[k]
        out[f"{tag}_nums"] = np.array([ref["user_num"], ref["item_num"], mine["rounds"]], dtype=np.int64)
        out[f"{tag}_dtypes"] = np.array([str(ref["user"].dtype), str(ref["item"].dtype)])
        print(f"{tag}: {len(cols['user'])} rows -> {len(ref['rows'])}, {ref['user_num']} users, {ref['item_num']} items, "
              f"{mine['rounds']} peel rounds: oracle == reference")
    assert out["stairs_nums"][2] >= 8, "the staircase must need at least 8 peel rounds"

    for tag, fx in O.SPLIT_FIXTURES.items():
        user, ts = O.split_frame(fx)
        df = pd.DataFrame({"user": user, "timestamp": ts})
        tr, te = RS.split_test(df.copy(), "tloo", uid="user", tid="timestamp")
        mtr, mte = O.split_tloo(user, ts)
        assert np.array_equal(tr, mtr) and np.array_equal(te, mte), tag
        out[f"{tag}_tloo_test"] = np.asarray(te, dtype=np.int64)
        for size in O.UTFO_SIZES:
            mtr, mte = O.split_utfo(user, size)
            if fx["contiguous"]:
                tr, te = RS.split_test(df.copy(), "utfo", size, uid="user")
                te = pd.Series(te).dropna().to_numpy().astype(np.int64)     # a user that contributes nothing explodes to NaN
                assert np.array_equal(np.asarray(tr).astype(np.int64), mtr) and np.array_equal(te, mte), (tag, size)
                out[f"{tag}_utfo_{size}_test"] = te
            np.random.seed(5)
            _, te = RS.split_test(df.copy(), "ufo", size, uid="user")
            counts = per_user_counts(user, te)
            assert np.array_equal(counts, per_user_counts(user, O.split_random("ufo", len(user), user, size)[1])), (tag, size)
            out[f"{tag}_ufo_{size}_counts"] = counts
            _, te = RS.split_test(df.copy(), "rsbr", size)
            assert len(te) == len(O.split_random("rsbr", len(user), None, size)[1])
            out[f"{tag}_rsbr_{size}_size"] = np.array(len(te))
        _, te = RS.split_test(df.copy(), "rloo", uid="user")
        assert len(te) == len(O.split_random("rloo", len(user), user)[1]) == len(np.unique(user))
        out[f"{tag}_rloo_size"] = np.array(len(te))
        print(f"{tag}: {len(user)} rows, {len(np.unique(user))} users: tloo, utfo, ufo counts, rsbr / rloo sizes equal")
    assert sorted(out["ufo_round_ufo_0.1_counts"]) == [0, 1, 2, 2, 3], "lengths 5, 10, 15, 25, 30 at 0.1"

    for n, size in O.TSBR_CASES:
        tr, te = RS.split_test(pd.DataFrame({"user": np.zeros(n, dtype=np.int64)}), "tsbr", size)
        mtr, mte = O.split_tsbr(n, size)
        assert np.array_equal(tr, mtr) and np.array_equal(te, mte)
        out[f"tsbr_{n}_{size}_split"] = np.array(len(tr))
    for n, k in O.CV_CASES:
        ref = list(KFold(n_splits=k).split(np.arange(n)))
        for f, ((tr, va), (mtr, mva)) in enumerate(zip(ref, O.split_cv(n, k))):
            assert np.array_equal(tr, mtr) and np.array_equal(va, mva), (n, k, f)
            out[f"cv_{n}_{k}_{f}_val"] = np.array([va[0], va[-1] + 1])
    try:
        list(RS.split_validation(pd.DataFrame({"user": np.zeros(10, dtype=np.int64)}), "cv", 3))
        out["cv_status"] = np.array("runs")
    except ValueError as e:
        out["cv_status"] = np.array("raises ValueError")
        print("reference cv:", e)
    path = os.path.join(HERE, "kat_prep.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
