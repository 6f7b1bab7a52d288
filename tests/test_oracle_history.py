"""tests/history_oracle.py against tests/golden/kat_history.npz (the real reference's get_history_matrix, AEDataset and
get_inter_matrix on every fixture), its two CSR routes against each other, and the four index_put_ rules of DESIGN.md §23,
each on a named row of the `edges` fixture.  Host only."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import history_oracle as O  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "kat_history.npz"))


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("name,row,use_value", O.CASES, ids=[O.case_id(*c) for c in O.CASES])
def test_padded_pair_equals_the_reference(name, row, use_value):
    tag, mine = O.case_id(name, row, use_value), O.expected(name, row, use_value)
    assert _same(mine["lens"], GOLD[f"{tag}_len"])
    assert mine["ids"].dtype == np.int64 and mine["vals"].dtype == np.float32
    if name in O.LARGE:
        assert mine["ids"].shape == tuple(GOLD[f"{tag}_shape"])
        assert O.digest(mine["ids"]) == str(GOLD[f"{tag}_ids_sha"]) and O.digest(mine["vals"]) == str(GOLD[f"{tag}_vals_sha"])
    else:
        assert _same(mine["ids"], GOLD[f"{tag}_ids"]) and _same(mine["vals"], GOLD[f"{tag}_vals"])


@pytest.mark.parametrize("name", list(O._BUILDERS))
def test_first_seen_and_coo_equal_the_reference(name):
    fx = O.fixture(name)
    for col in ("user", "item"):
        assert _same(O.first_seen(fx[col]), GOLD[f"{name}_first_{col}"])
    for k, a in zip(("row", "col", "data"), O.coo_columns(fx)):
        if name in O.LARGE:
            assert O.digest(a) == str(GOLD[f"{name}_coo_{k}_sha"])
        else:
            assert _same(a, GOLD[f"{name}_coo_{k}"])


def test_the_tiny_fixture_is_the_one_the_design_quotes():
    e = O.expected("tiny", "user", True)
    assert e["ids"].tolist() == [[0, 1, 0], [0, 3, 0], [0, 0, 0], [0, 2, 0], [0, 0, 0]]
    assert e["vals"].tolist() == [[4, 3, 0], [2, 2.5, 0], [0, 0, 0], [5, 0, 1], [0, 0, 0]]
    assert e["lens"].tolist() == [2, 2, 0, 3, 0]
    assert O.first_seen(O.fixture("tiny")["user"]).tolist() == [3, 0, 1]
    assert O.coo_columns(O.fixture("tiny"))[0].tolist() == [3, 0, 3, 1, 0, 3, 1]
    row_ptr, col, val, L = e["csr"]
    # users 0 and 1 are short and lose item 0; user 3 is the longest: item 0 stays with its last value, item 2 (value 0) goes
    assert (row_ptr.tolist(), col.tolist(), val.tolist(), L) == ([0, 1, 2, 2, 3, 3], [1, 3, 0], [3.0, 2.5, 1.0], 3)


@pytest.mark.parametrize("name,row,use_value", O.CASES, ids=[O.case_id(*c) for c in O.CASES])
def test_dense_rows_then_nonzeros_equal_the_direct_csr(name, row, use_value):
    e = O.expected(name, row, use_value)
    _, _, _, R, Cn = O.columns(O.fixture(name), row, use_value)
    via_dense = O.csr_of_dense(O.dense_rows(e["ids"], e["vals"], Cn))
    row_ptr, col, val, L = e["csr"]
    assert L == e["ids"].shape[1] and row_ptr.shape == (R + 1,)
    assert _same(via_dense[0], row_ptr) and _same(via_dense[1], col) and _same(via_dense[2], val)
    assert col.dtype == np.int32 and val.dtype == np.float32 and row_ptr.dtype == np.int64


def _row(csr, r):
    row_ptr, col, val, _ = csr
    return dict(zip(col[row_ptr[r]:row_ptr[r + 1]].tolist(), val[row_ptr[r]:row_ptr[r + 1]].tolist()))


@pytest.mark.parametrize("name,row", [("edges_mixed_u", "user"), ("edges_contig_u", "user"), ("edges_mixed_i", "item"),
                                      ("edges_contig_i", "item")])
def test_each_index_put_rule_on_its_named_row(name, row):
    e = O.expected(name, row, True)
    lens, csr = e["lens"], e["csr"]
    assert sorted(set(lens.tolist())) == [0, 1, 2, 3, 7, 63, 64, 65, O.LONGEST] and csr[3] == O.LONGEST
    assert np.flatnonzero(lens == O.LONGEST).tolist() == [O.ROW_LAST_WINS, O.ROW_TIED_KEEPS_0]
    assert O.LONGEST > O.COL_NUM        # duplicates are forced
    # 1. of a duplicated pair the last one in frame order stays
    assert _row(csr, O.ROW_LAST_WINS)[7] == 4.0
    # 2. a row shorter than the longest loses its column 0
    assert lens[O.ROW_SHORT_LOSES_0] == 63 and 0 in e["ids"][O.ROW_SHORT_LOSES_0, :63]
    assert 0 not in _row(csr, O.ROW_SHORT_LOSES_0)
    assert lens[O.ROW_ONLY_0] == 1 and _row(csr, O.ROW_ONLY_0) == {}
    # 3. a row as long as the longest keeps it, and so does the row tied with it
    assert _row(csr, O.ROW_LAST_WINS)[0] == 3.5 and _row(csr, O.ROW_TIED_KEEPS_0)[0] == 3.0
    # 4. entries whose float32 value is 0 are dropped: an exact zero, a float64 that rounds to zero; a zero followed by
    #    a value is kept, rounded to float32 once
    z = _row(csr, O.ROW_ZERO_DROPPED)
    assert 9 not in z and 11 not in z and z[13] == float(np.float32(O.INEXACT)) != O.INEXACT
    # without the value column every entry is 1.0: only the padding rule removes anything
    ones = O.expected(name, row, False)["csr"]
    assert set(ones[2].tolist()) == {1.0} and 9 in _row(ones, O.ROW_ZERO_DROPPED) and 0 not in _row(ones, O.ROW_SHORT_LOSES_0)
    # several short rows hold column 0
    assert sum(1 for r in range(O.ROW_NUM) if 0 < lens[r] < O.LONGEST and 0 in e["ids"][r, :lens[r]]) >= 5
