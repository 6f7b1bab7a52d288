"""tests/prep_oracle.py against the stored reference values (tests/golden/kat_prep.npz, written by
tests/golden/make_golden_prep.py from the real daisy.utils.loader / daisy.utils.splitter): every comparison is exact."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import prep_oracle as O  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "kat_prep.npz"))
GOLDEN_TAGS = [t for t, fx in O.PREP_FIXTURES.items() if not fx.get("ties")]


def _tokens(t):
    t = np.asarray(t)
    return t.astype(str) if t.dtype == object else t


@pytest.mark.parametrize("tag", GOLDEN_TAGS)
def test_process_equals_the_reference(tag):
    fx = O.PREP_FIXTURES[tag]
    c = O.prep_frame(fx)
    got = O.process(c["user"], c["item"], c["rating"], c["timestamp"], fx["prepro"], fx["level"], fx.get("threshold"))
    for k in ("rows", "user", "item", "item_pop"):
        want = GOLD[f"{tag}_{k}"]
        assert got[k].dtype == want.dtype and np.array_equal(got[k], want), (tag, k)
    assert [str(got["user"].dtype), str(got["item"].dtype)] == list(GOLD[f"{tag}_dtypes"])
    assert np.array_equal(_tokens(got["uid_token"]), GOLD[f"{tag}_uid_token"])
    assert np.array_equal(_tokens(got["iid_token"]), GOLD[f"{tag}_iid_token"])
    assert [got["user_num"], got["item_num"], got["rounds"]] == list(GOLD[f"{tag}_nums"])


def test_fixture_properties():
    assert GOLD["stairs_nums"][2] >= 8
    assert str(GOLD["empty_status"]) == "returns an empty frame" and list(GOLD["empty_nums"][:2]) == [0, 0]
    assert [str(GOLD[f"users{k}_dtypes"][0]) for k in (126, 127, 128, 129)] == ["int8", "int16", "int16", "int16"]
    c = O.prep_frame(O.PREP_FIXTURES["triple"])
    rows = [5, 120, 290]
    assert len({(c["user"][r], c["item"][r]) for r in rows}) == 1 and c["rating"][290] == 3.0
    kept = GOLD["triple_rows"]
    assert 290 in kept and 5 not in kept and 120 not in kept          # the last copy, whose rating equals the threshold
    c = O.prep_frame(O.PREP_FIXTURES["thresh"])
    assert np.isnan(c["rating"]).any() and not np.isnan(c["rating"][GOLD["thresh_rows"]]).any()
    for tag, col in (("hotitem", "item"), ("hotuser", "user")):
        c = O.prep_frame(O.PREP_FIXTURES[tag])
        assert np.bincount(c[col]).max() >= len(c[col]) // 2
    assert str(GOLD["cv_status"]) in ("runs", "raises ValueError")


def test_philox_is_the_library_generator():
    sys.path.insert(0, os.path.dirname(HERE))
    from oracle import bpr_mf_numpy as B
    idx = np.array([0, 1, 2, 255, 2 ** 31 - 1, 2 ** 32 + 7], dtype=np.uint64)
    for seed, stream in ((2022, O.SPLIT_STREAM), (0, O.SPLIT_STREAM | 3), (2 ** 40 + 5, 1)):
        got = O.philox_u64(seed, stream, idx)
        assert [int(x) for x in got] == [B._draw_u64(seed, stream, int(i)) for i in idx]


@pytest.mark.parametrize("tag", list(O.SPLIT_FIXTURES))
def test_splits_equal_the_reference(tag):
    fx = O.SPLIT_FIXTURES[tag]
    user, ts = O.split_frame(fx)
    n = len(user)
    tr, te = O.split_tloo(user, ts)
    assert np.array_equal(te, GOLD[f"{tag}_tloo_test"]) and np.array_equal(tr, np.setdiff1d(np.arange(n), te))
    tok = np.unique(user)
    for size in O.UTFO_SIZES:
        tr, te = O.split_utfo(user, size)
        if fx["contiguous"]:
            assert np.array_equal(te, GOLD[f"{tag}_utfo_{size}_test"])
        lens = np.bincount(np.searchsorted(tok, user))
        want = lens - np.array([int(np.ceil(l * (1 - size))) for l in lens])
        assert np.array_equal(np.bincount(np.searchsorted(tok, user[te]), minlength=len(tok)), want)
        _, te = O.split_random("ufo", n, user, size)
        assert np.array_equal(np.bincount(np.searchsorted(tok, user[te]), minlength=len(tok)), GOLD[f"{tag}_ufo_{size}_counts"])
        assert len(O.split_random("rsbr", n, None, size)[1]) == int(GOLD[f"{tag}_rsbr_{size}_size"])
    assert len(O.split_random("rloo", n, user)[1]) == int(GOLD[f"{tag}_rloo_size"])


def test_tsbr_and_cv():
    for n, size in O.TSBR_CASES:
        tr, te = O.split_tsbr(n, size)
        k = int(GOLD[f"tsbr_{n}_{size}_split"])
        assert np.array_equal(tr, np.arange(k)) and np.array_equal(te, np.arange(k, n))
    for n, k in O.CV_CASES:
        for f, (tr, va) in enumerate(O.split_cv(n, k)):
            a, b = GOLD[f"cv_{n}_{k}_{f}_val"]
            assert np.array_equal(va, np.arange(a, b)) and np.array_equal(tr, np.setdiff1d(np.arange(n), va))
