"""`daisyrec_amd.utils.loader.Preprocessor` on the device against the stored reference values (tests/golden/kat_prep.npz)
and, where the reference cannot serve (timestamp ties), against tests/prep_oracle.py.  Every comparison is exact, dtypes
included.  The oracle results are computed once per fixture and shared."""
import functools
import logging
import os
import sys

import numpy as np
import pandas as pd
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import prep_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(HERE, "golden", "kat_prep.npz"))


def _config(fx, **over):
    cfg = {"dataset": "fixture", "prepro": fx["prepro"], "UID_NAME": "user", "IID_NAME": "item", "TID_NAME": "timestamp",
           "INTER_NAME": "rating", "binary_inter": True, "positive_threshold": fx.get("threshold"), "level": fx["level"],
           "logger": logging.getLogger("test"), "metrics": ["popularity"]}
    cfg.update(over)
    return cfg


@functools.lru_cache(maxsize=None)
def _frame(tag):
    c = O.prep_frame(O.PREP_FIXTURES[tag])
    df = pd.DataFrame({k: c[k] for k in ("user", "item", "rating", "timestamp")})
    df["row"] = np.arange(len(df), dtype=np.int64)
    return df


@functools.lru_cache(maxsize=None)
def _oracle(tag):
    fx, df = O.PREP_FIXTURES[tag], _frame(tag)
    return O.process(df["user"].to_numpy(), df["item"].to_numpy(), df["rating"].to_numpy(), df["timestamp"].to_numpy(),
                     fx["prepro"], fx["level"], fx.get("threshold"))


def _run(tag, **over):
    from daisyrec_amd.utils.loader import Preprocessor
    p = Preprocessor(_config(O.PREP_FIXTURES[tag], **over))
    return p, p.process(_frame(tag))


def _tokens(t):
    t = np.asarray(t)
    return t.astype(str) if t.dtype == object else t


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and np.array_equal(a, b)


def _check(p, out, want, tag):
    """want: rows, user, item, uid_token, iid_token, item_pop, user_num, item_num"""
    assert list(out.columns) == ["user", "item", "rating", "timestamp", "row"]
    assert isinstance(out.index, pd.RangeIndex) and out.index.start == 0 and len(out) == len(want["rows"])
    assert _same(out["row"].to_numpy(), want["rows"]), tag
    assert _same(out["user"].to_numpy(), want["user"]) and _same(out["item"].to_numpy(), want["item"]), tag
    src = _frame(tag)
    assert np.array_equal(out["timestamp"].to_numpy(), src["timestamp"].to_numpy()[want["rows"]])
    assert out["rating"].dtype == np.float64 and (out["rating"] == 1.0).all()
    assert np.array_equal(_tokens(p.uid_token), _tokens(want["uid_token"])), tag
    assert np.array_equal(_tokens(p.iid_token), _tokens(want["iid_token"])), tag
    assert _same(p.item_pop, want["item_pop"]), tag
    assert (p.user_num, p.item_num) == (want["user_num"], want["item_num"]) == (p.get_user_num(), p.get_item_num())
    assert p.token_uid == {t: k for k, t in enumerate(p.uid_token)} and len(p.token_iid) == p.item_num


GOLDEN_TAGS = [t for t, fx in O.PREP_FIXTURES.items() if not fx.get("ties")]
TIE_TAGS = [t for t, fx in O.PREP_FIXTURES.items() if fx.get("ties")]


@pytest.mark.parametrize("tag", GOLDEN_TAGS)
def test_process_equals_the_reference(tag):
    p, out = _run(tag)
    nums = GOLD[f"{tag}_nums"]
    want = {k: GOLD[f"{tag}_{k}"] for k in ("rows", "user", "item", "uid_token", "iid_token", "item_pop")}
    want.update(user_num=int(nums[0]), item_num=int(nums[1]))
    _check(p, out, want, tag)
    assert [str(out["user"].dtype), str(out["item"].dtype)] == list(GOLD[f"{tag}_dtypes"])
    assert p.rounds == int(nums[2]) == _oracle(tag)["rounds"]


@pytest.mark.parametrize("tag", TIE_TAGS)
def test_ties_stay_in_input_order(tag):
    """heavy timestamp ties on either side of the size at which the id sorts change algorithm: the stable order"""
    p, out = _run(tag)
    want = _oracle(tag)
    _check(p, out, want, tag)
    assert p.rounds == want["rounds"]
    ts, row = out["timestamp"].to_numpy(), out["row"].to_numpy()
    assert (np.diff(ts) >= 0).all() and (np.diff(row)[np.diff(ts) == 0] > 0).all()


def test_staircase_round_count():
    p, out = _run("stairs")
    assert p.rounds == _oracle("stairs")["rounds"] >= 8 and len(out) == 9


def test_empty_core_is_an_empty_frame():
    p, out = _run("empty")
    assert len(out) == 0 and p.user_num == 0 and p.item_num == 0 and p.uid_token.size == 0 and p.token_uid == {}
    assert list(out.columns) == ["user", "item", "rating", "timestamp", "row"] and p.item_pop.shape == (0,)


def test_two_calls_give_identical_bytes():
    for tag in ("hotitem", "ties_small"):
        (p1, a), (p2, b) = _run(tag), _run(tag)
        for col in a.columns:
            assert a[col].to_numpy().tobytes() == b[col].to_numpy().tobytes(), (tag, col)
        assert p1.item_pop.tobytes() == p2.item_pop.tobytes() and p1.uid_token.tobytes() == p2.uid_token.tobytes()


def test_options_and_column_types():
    tag = "3core_ui"
    want = _oracle(tag)
    # no popularity asked, ratings kept, a datetime64 timestamp, int32 ids, a further column carried along
    from daisyrec_amd.utils.loader import Preprocessor
    df = _frame(tag).copy()
    df["timestamp"] = pd.to_datetime(df["timestamp"] + 10 ** 6, unit="s")
    df["user"], df["item"] = df["user"].astype(np.int32), df["item"].astype(np.int16)
    p = Preprocessor(_config(O.PREP_FIXTURES[tag], metrics=["ndcg"], binary_inter=False))
    out = p.process(df)
    assert p.item_pop is None and _same(out["row"].to_numpy(), want["rows"])
    assert np.array_equal(out["rating"].to_numpy(), df["rating"].to_numpy()[want["rows"]])
    assert out["timestamp"].dtype == df["timestamp"].dtype and p.uid_token.dtype == np.int32
    assert _same(out["user"].to_numpy(), want["user"]) and _same(out["item"].to_numpy(), want["item"])
    assert list(df.columns) == list(_frame(tag).columns) and len(df) == 1000          # the input is left alone
