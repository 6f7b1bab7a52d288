"""tests/rank_positions_oracle.py against the lists the REAL reference's MF.full_rank / FM.full_rank produced
(tests/golden/kat_full_rank.npz), its KPI formulas against tests/metrics_oracle.py on explicit lists, and the argument
checks and workspace sizes of daisy_full_rank_positions / daisy_position_kpis.  CPU only."""
import ctypes
import os
import re

import numpy as np
import pytest

import metrics_oracle as MO
import rank_positions_oracle as RO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(HERE, "golden", "kat_full_rank.npz"))


@pytest.mark.parametrize("model", ["mf", "fm"])
def test_a_listed_item_has_its_list_index_as_position(kat, model):
    P, Q = kat["P"], kat["Q"]
    users = np.arange(P.shape[0])
    lists = kat[f"full_{model}"]
    biases = (kat["bu"], kat["bi"], kat["b0"]) if model == "fm" else None
    targets = {int(u): set(lists[u].tolist()) for u in users}
    out_indptr, pos, sc, eligible, _ = RO.positions_exact(P, Q, users, targets, biases=biases)
    assert np.all(eligible == Q.shape[0]) and out_indptr[-1] == lists.size
    for u in users:
        row = np.sort(lists[u])
        p = pos[out_indptr[u]:out_indptr[u + 1]]
        assert np.array_equal(lists[u][p], row), u              # the item at index pos is the target
    # and under an exclusion: dropping the first three of a list moves the others up by three
    excl = {0: set(lists[0, :3].tolist())}
    _, pos_x, sc_x, el_x, _ = RO.positions_exact(P, Q, np.array([0]), targets, exclude=excl, biases=biases)
    row = np.sort(lists[0])
    want = np.array([-1 if t in excl[0] else lists[0].tolist().index(t) - 3 for t in row.tolist()])
    assert np.array_equal(pos_x, want) and el_x[0] == Q.shape[0] - 3
    assert np.all(np.isneginf(sc_x[want < 0])) and np.all(np.isfinite(sc_x[want >= 0]))


def test_ties_out_of_range_targets_and_bounds():
    P = np.zeros((3, 4), np.float32)
    Q = np.zeros((9, 4), np.float32)
    targets = {0: {1, 5, 8, 20}, 1: set(), 2: {0}}
    out_indptr, pos, sc, el, lists = RO.positions_exact(P, Q, np.array([0, 1, 2, 0]), targets, exclude={0: {0, 5}})
    assert out_indptr.tolist() == [0, 4, 4, 5, 9] and el.tolist() == [7, 9, 9, 7]
    assert pos.tolist() == [0, -1, 6, -1, 0, 0, -1, 6, -1]      # all scores equal: the eligible ids below the target
    rng = np.random.default_rng(5)
    P = rng.normal(0, 0.1, (6, 64)).astype(np.float32)
    Q = rng.normal(0, 0.1, (200, 64)).astype(np.float32)
    users = np.arange(6)
    targets = {u: set(rng.choice(200, 5, replace=False).tolist()) for u in range(6)}
    s32 = (P @ Q.T).astype(np.float32)
    _, pos, _, _, _ = RO.positions(s32, users, targets)
    lo, hi = RO.position_bounds(P, Q, users, targets)
    assert np.all((lo <= pos) & (pos <= hi)) and np.all(hi - lo <= 2)


@pytest.mark.parametrize("seed", range(4))
def test_closed_forms_equal_the_list_kpis(seed):
    """random hit patterns, K above len(gt), above the eligible items, no hit and all hits"""
    rng = np.random.default_rng(seed)
    metrics = list(RO.LIST_KPIS) + ["full_auc"]
    cutoffs = [1, 3, 10, 40, 200]
    E = [60, 60, 60, 25, 7, 60]
    rows = [rng.choice(60, 6, replace=False), np.arange(4) + 50, np.arange(5), rng.choice(25, 9, replace=False),
            np.arange(7), rng.choice(60, 60, replace=False)]        # random, no hit below 50, all hits, K > E, row = list
    pos = [np.where(rng.random(r.size) < 0.2, -1, r) if b == 0 else r for b, r in enumerate(rows)]
    out_indptr = np.concatenate([[0], np.cumsum([len(p) for p in pos])])
    flat = np.concatenate(pos).astype(np.int32)
    per, means = RO.kpis_from_positions(out_indptr, flat, None, E, cutoffs, metrics)
    for b in range(len(rows)):
        for c, K in enumerate(cutoffs):
            for m in metrics:
                got, want = RO.closed_form(pos[b], len(pos[b]), E[b], K, m), per[m][c, b]
                if m in MO.BITWISE or m in ("full_auc", "f1", "map"):
                    assert np.array_equal(got, want, equal_nan=True), (b, K, m, got, want)
                else:
                    assert abs(got - want) <= 4 * len(pos[b]) * MO.U64 * abs(want), (b, K, m, got, want)
    assert np.isnan(per["auc"][4, 4]) and np.isnan(per["full_auc"][0, 4])       # every eligible item is a target: 0 / 0
    assert per["precision"][4, 3] == 9 / 25                                     # K = 200 over 25 eligible items


def _header_args(name):
    src = open(os.path.join(ROOT, "include", "daisyrec_amd.h")).read()
    m = re.search(r"\b%s\(([^;]*)\);" % name, src)
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


def test_signatures_follow_the_header():
    from daisyrec_amd import _native as N
    kinds = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32}
    for name in ("daisy_full_rank_positions", "daisy_full_rank_positions_workspace_bytes", "daisy_position_kpis",
                 "daisy_position_kpis_workspace_bytes"):
        want = []
        for a in _header_args(name):
            if "*" in a or a.startswith("daisy_stream_t"):
                want.append(ctypes.POINTER(ctypes.c_int32) if "cutoffs_host" in a else ctypes.c_void_p)
            else:
                want.append(kinds[a.split()[0]])
        assert N.SIGNATURES[name][1] == want, name


def _call(N, buf, **over):
    d = ctypes.addressof(buf)
    a = dict(P=d, Q=d, bu=None, bi=None, b0=None, d=16, I=1000, users=d, n=4, indptr=None, items=None, tp=d, ti=d, op=d, T=40,
             slices=0, pos=d, scores=None, elig=None, ws=d, ws_bytes=1 << 40)
    a.update(over)
    return N.lib.daisy_full_rank_positions(a["P"], a["Q"], a["bu"], a["bi"], a["b0"], a["d"], a["I"], a["users"], a["n"],
                                           a["indptr"], a["items"], a["tp"], a["ti"], a["op"], a["T"], a["slices"], a["pos"],
                                           a["scores"], a["elig"], a["ws"], a["ws_bytes"], None)


def test_argument_errors_do_not_need_a_gpu():
    """every check precedes the first HIP call (the pointers are dummies nobody reads)"""
    from daisyrec_amd import _native as N
    buf = ctypes.create_string_buffer(256)
    d = ctypes.addressof(buf)
    cases = [(dict(P=None), "NULL"), (dict(Q=None), "NULL"), (dict(users=None), "NULL"), (dict(tp=None), "NULL"),
             (dict(ti=None), "NULL"), (dict(op=None), "NULL"), (dict(pos=None), "NULL"), (dict(ws=None), "NULL"),
             (dict(d=100000), "d=100000"), (dict(d=0), "d=0"), (dict(indptr=d), "excl_indptr"), (dict(items=d), "excl_indptr"),
             (dict(bu=d), "u_bias"), (dict(bu=d, bi=d), "u_bias"), (dict(n=0), "n=0"), (dict(T=-1), "n_targets=-1"),
             (dict(I=0), "item_num=0"), (dict(I=1 << 31), "item_num="), (dict(slices=-1), "item_slices"),
             (dict(ws_bytes=8), "workspace")]
    for over, text in cases:
        rc = _call(N, buf, **over)
        assert rc == N.DAISY_ERR_ARG, (over, rc)
        msg = N.last_error()
        assert msg.startswith("full_rank_positions:") and text in msg, (over, msg)
    cut = (ctypes.c_int32 * 3)(1, 5, 500)

    def kpis(**over):
        a = dict(op=d, pos=d, gl=None, el=d, n=4, cut=cut, nc=3, disc=d, cum=d, dl=10, mask=0b11111111, pu=None, means=d, ws=d,
                 ws_bytes=1 << 30)
        a.update(over)
        return N.lib.daisy_position_kpis(a["op"], a["pos"], a["gl"], a["el"], a["n"], a["cut"], a["nc"], a["disc"], a["cum"],
                                         a["dl"], a["mask"], a["pu"], a["means"], a["ws"], a["ws_bytes"], None)
    bad = (ctypes.c_int32 * 3)(1, 5, 5)
    for over, text in [(dict(op=None), "NULL"), (dict(el=None), "NULL"), (dict(means=None), "NULL"), (dict(n=0), "n=0"),
                       (dict(nc=0), "cutoffs"), (dict(nc=13), "cutoffs"), (dict(cut=bad), "strictly ascending"),
                       (dict(mask=0), "metrics mask"), (dict(mask=1 << 8), "need the lists"), (dict(mask=1 << 10), "need the lists"),
                       (dict(disc=None), "ndcg"), (dict(ws_bytes=8), "workspace")]:
        rc = kpis(**over)
        assert rc == N.DAISY_ERR_ARG, (over, rc)
        msg = N.last_error()
        assert msg.startswith("position_kpis:") and text in msg, (over, msg)


def test_workspaces():
    from daisyrec_amd import _native as N
    ws = N.lib.daisy_full_rank_positions_workspace_bytes
    up = lambda x: (x + 255) // 256 * 256         # noqa: E731
    # a sort word per target, two int64 per slot (at most n + T / 32 of them) and one per block of 256 requests
    assert ws(100, 1000) == up(1000 * 8) + 2 * up((100 + 1000 // 32) * 8) + up(8)
    assert ws(1000, 0) == up(8) + 2 * up(1000 * 8) + up(4 * 8)
    assert ws(0, 10) == 0 and ws(10, -1) == 0
    n, T, I = 1 << 20, 10 << 20, 1 << 17
    assert 0 < ws(n, T) < n * I * 4 // 1000
    kw = N.lib.daisy_position_kpis_workspace_bytes
    assert kw(1000, 3, 0b11) == up(2 * 3 * 4 * 8) and kw(1000, 3, 1 << N.KPI_FULL_AUC) == up(3 * 4 * 8)
    assert kw(0, 3, 1) == 0 and kw(10, 13, 1) == 0 and kw(10, 3, 1 << 9) == 0 and kw(10, 3, 0) == 0
