"""`get_history_matrix`, `history_csr`, `AEDataset` and `get_inter_matrix` on the device (csrc/history.hip)
against the stored reference values (tests/golden/kat_history.npz) and tests/history_oracle.py, and the models that take
their results: VAECF from config['history_csr'], LightGCN / NGCF from the device inter-matrix.  Every comparison is exact,
dtypes included.  The oracle's answers are computed once per case and shared; nothing here reads the reference checkout."""
import functools
import gc
import logging
import os
import sys

import numpy as np
import pandas as pd
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import history_oracle as O  # noqa: E402
from conftest import mf_config  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(HERE, "golden", "kat_history.npz"))
CASE_IDS = [O.case_id(*c) for c in O.CASES]


def _config(fx, **over):
    cfg = {"UID_NAME": "user", "IID_NAME": "item", "INTER_NAME": "rating", "user_num": fx["user_num"],
           "item_num": fx["item_num"], "logger": logging.getLogger("test")}
    cfg.update(over)
    return cfg


@functools.lru_cache(maxsize=None)
def _frame(name):
    fx = O.fixture(name)
    return pd.DataFrame({"user": fx["user"], "item": fx["item"], "rating": fx["rating"]})


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _host(t):
    assert t.is_cuda
    return t.cpu().numpy()


def _csr_equal(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w) for g, w in zip(got[:3], want[:3]))


@pytest.mark.parametrize("name,row,use_value", O.CASES, ids=CASE_IDS)
def test_padded_pair_and_direct_csr(name, row, use_value):
    from daisyrec_amd import ops
    from daisyrec_amd.utils import utils as U
    fx, df, tag = O.fixture(name), _frame(name), O.case_id(name, row, use_value)
    want = O.expected(name, row, use_value)
    _, _, _, R, Cn = O.columns(fx, row, use_value)
    ids, vals, lens = U.get_history_matrix(df, _config(fx), row=row, use_config_value_name=use_value)
    L = want["ids"].shape[1]
    assert (ids.dtype, vals.dtype, lens.dtype) == (torch.int64, torch.float32, torch.int64)
    assert (tuple(ids.shape), tuple(vals.shape), tuple(lens.shape)) == ((R, L), (R, L), (R,))
    assert ids.is_cuda and vals.is_cuda and lens.is_cuda and ids.is_contiguous() and vals.is_contiguous()
    assert _same(_host(lens), GOLD[f"{tag}_len"])
    if name in O.LARGE:
        assert tuple(ids.shape) == tuple(GOLD[f"{tag}_shape"])
        assert O.digest(_host(ids)) == str(GOLD[f"{tag}_ids_sha"]) and O.digest(_host(vals)) == str(GOLD[f"{tag}_vals_sha"])
    else:
        assert _same(_host(ids), GOLD[f"{tag}_ids"]) and _same(_host(vals), GOLD[f"{tag}_vals"])
    # the direct CSR: the oracle's, and what the torch route makes of the padded pair
    csr = U.history_csr(df, _config(fx), row=row, use_config_value_name=use_value)
    assert csr[3] == L == want["csr"][3]
    for got, exp in zip(csr[:3], want["csr"][:3]):
        assert _same(_host(got), exp)
    assert _csr_equal(csr, ops.vae_history_csr(ids, vals, Cn))
    # two calls give identical bytes
    again = U.get_history_matrix(df, _config(fx), row=row, use_config_value_name=use_value)
    assert torch.equal(again[0], ids) and torch.equal(again[1].view(torch.int32), vals.view(torch.int32))
    assert torch.equal(again[2], lens)
    csr2 = U.history_csr(df, _config(fx), row=row, use_config_value_name=use_value)
    assert csr2[3] == csr[3] and torch.equal(csr2[0], csr[0]) and torch.equal(csr2[1], csr[1])
    assert torch.equal(csr2[2].view(torch.int32), csr[2].view(torch.int32))


@pytest.mark.parametrize("name", list(O._BUILDERS))
def test_first_seen_order_and_inter_matrix(name):
    from daisyrec_amd.utils import utils as U
    from daisyrec_amd.utils.dataset import AEDataset
    fx, df = O.fixture(name), _frame(name)
    for col in ("user", "item"):
        ds = AEDataset(df, yield_col=col)
        assert isinstance(ds.data, np.ndarray) and _same(ds.data, GOLD[f"{name}_first_{col}"])
        assert len(ds) == len(ds.data) and (len(ds) == 0 or ds[0] == ds.data[0])
        assert _same(AEDataset(df, yield_col=col).data, ds.data)
    m = U.get_inter_matrix(df, _config(fx))
    assert m.tocoo() is m and m.shape == (fx["user_num"], fx["item_num"]) and m.nnz == len(df)
    assert (m.row.dtype, m.col.dtype, m.data.dtype) == (torch.int32, torch.int32, torch.float64)
    for k, t in (("row", m.row), ("col", m.col), ("data", m.data)):
        if name in O.LARGE:
            assert O.digest(_host(t)) == str(GOLD[f"{name}_coo_{k}_sha"])
        else:
            assert _same(_host(t), GOLD[f"{name}_coo_{k}"])


def test_first_seen_of_raw_ids_and_scipy_forms():
    """ids that are no dense codes (negative, far apart) take the encode route; 'csr' is scipy's CSR of the same frame"""
    sp = pytest.importorskip("scipy.sparse")
    from daisyrec_amd.utils import utils as U
    from daisyrec_amd.utils.dataset import AEDataset
    fx = O.fixture("edges_mixed_u")
    raw = fx["user"] * 1_000_000_007 - 5_000_000_000
    assert _same(AEDataset(pd.DataFrame({"user": raw})).data, O.first_seen(raw))
    df = _frame("edges_mixed_u")
    want = sp.coo_matrix((fx["rating"], (fx["user"], fx["item"])), shape=(fx["user_num"], fx["item_num"]))
    got = U.get_inter_matrix(df, _config(fx)).to_scipy()
    assert sp.isspmatrix_coo(got) and _same(got.row, want.row) and _same(got.col, want.col) and _same(got.data, want.data)
    csr, wcsr = U.get_inter_matrix(df, _config(fx), "csr"), want.tocsr()
    assert sp.isspmatrix_csr(csr) and _same(csr.indptr, wcsr.indptr) and _same(csr.indices, wcsr.indices)
    assert _same(csr.data, wcsr.data)


def test_log_line_when_a_row_holds_a_fifth_of_the_columns(caplog):
    from daisyrec_amd.utils import utils as U
    fx = O.fixture("tiny")
    with caplog.at_level(logging.INFO, logger="test"):
        U.get_history_matrix(_frame("tiny"), _config(fx))
    assert "Max value of user's history interaction records has reached: 75.0000% of the total." in caplog.text
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="test"):
        U.get_history_matrix(_frame("tiny"), _config(fx, item_num=15))       # 3 == 0.2 * 15: not above
    assert "Max value" not in caplog.text


@pytest.mark.parametrize("name,row", [("edges_mixed_u", "user"), ("edges_contig_i", "item"), ("tiny", "user")])
def test_rating_rows_from_device_built_tensors(name, row):
    """AERecommender.get_user_rating_matrix / get_item_rating_matrix on the device tensors == the oracle's dense rows"""
    from daisyrec_amd.model.AbstractRecommender import AERecommender
    from daisyrec_amd.utils import utils as U
    fx = O.fixture(name)
    ids, vals, _ = U.get_history_matrix(_frame(name), _config(fx), row=row, use_config_value_name=True)
    want = O.expected(name, row, True)
    _, _, _, R, Cn = O.columns(fx, row, True)
    m = AERecommender(mf_config())
    m.user_num, m.item_num = fx["user_num"], fx["item_num"]
    if row == "user":
        m.history_item_id, m.history_item_value = ids, vals
        got = m.get_user_rating_matrix(torch.arange(R))
    else:
        m.history_user_id, m.history_user_value = ids, vals
        got = m.get_item_rating_matrix(torch.arange(R))
    assert _same(_host(got), O.dense_rows(want["ids"], want["vals"], Cn))


# ---- VAECF from config['history_csr'] ------------------------------------------------------------------------------------
def _vae(fx, **over):
    from daisyrec_amd.model import VAECF
    torch.manual_seed(3)
    cfg = mf_config(algo_name="multi-vae", mlp_hidden_size=[16], epochs=2, dropout=0.5, lr=0.001, latent_dim=8,
                    total_anneal_steps=100, anneal_cap=0.2, topk=10, user_num=fx["user_num"], item_num=fx["item_num"])
    cfg.update(over)
    return VAECF(cfg)


def test_vaecf_from_the_csr_is_the_fit_from_the_padded_pair():
    from daisyrec_amd.utils import utils as U
    from daisyrec_amd.utils.dataset import AEDataset, CandidatesDataset, get_dataloader
    from torch.utils.data import DataLoader
    name = "edges_mixed_u"
    fx, df = O.fixture(name), _frame(name)
    ids, vals, _ = U.get_history_matrix(df, _config(fx), row="user", use_config_value_name=True)
    csr = U.history_csr(df, _config(fx), row="user", use_config_value_name=True)
    train = AEDataset(df, yield_col="user")
    rng = np.random.default_rng(0)
    users = np.arange(0, fx["user_num"], 3)
    ucands = [[int(u), rng.integers(0, fx["item_num"], 40)] for u in users]
    outs = []
    for kw in (dict(history_item_id=ids, history_item_value=vals),
               dict(history_item_id=None, history_item_value=None, history_csr=csr)):
        m = _vae(fx, **kw)
        g = torch.Generator()
        g.manual_seed(5)
        m.fit(DataLoader(train, batch_size=32, shuffle=True, generator=g))
        ranks = m.rank(get_dataloader(CandidatesDataset(ucands), batch_size=8, shuffle=False, num_workers=0))
        full = [m.full_rank(int(u)) for u in (0, 6, 69)]
        preds = [m.predict(int(u), int(i)) for u, i in ((0, 7), (3, 0), (69, 129))]
        dense = m.get_user_rating_matrix(torch.arange(fx["user_num"]))
        outs.append((list(m.epoch_losses), m._params().clone(), ranks, full, preds, dense))
    (la, wa, ra, fa, pa, da), (lb, wb, rb, fb, pb, db) = outs
    assert len(la) == 2 and all(np.isfinite(la)) and la == lb
    assert torch.equal(wa.view(torch.int32), wb.view(torch.int32))
    assert _same(ra, rb) and all(_same(x, y) for x, y in zip(fa, fb)) and pa == pb
    assert torch.equal(da, db) and _same(_host(db), O.dense_rows(*(O.expected(name, "user", True)[k] for k in ("ids", "vals")),
                                                               fx["item_num"]))
    m = _vae(fx, history_item_id=None, history_item_value=None, history_csr=csr)
    with pytest.raises(IndexError, match="index 70 is out of bounds for dimension 0 with size 70"):
        m.full_rank(70)
    with pytest.raises(IndexError, match="history item ids must lie in"):
        _vae(fx, item_num=100, history_item_id=None, history_item_value=None, history_csr=csr).full_rank(0)


# ---- LightGCN / NGCF from the device inter-matrix ------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["lightgcn", "ngcf"])
def test_graph_models_from_the_device_inter_matrix(algo):
    sp = pytest.importorskip("scipy.sparse")
    from daisyrec_amd.model import LightGCN, NGCF
    from daisyrec_amd.utils import utils as U
    from daisyrec_amd.utils.dataset import BasicDataset, get_dataloader
    fx, df = O.fixture("edges_mixed_u"), _frame("edges_mixed_u")
    Un, In = fx["user_num"], fx["item_num"]
    rng = np.random.default_rng(4)
    samples = np.stack([fx["user"], fx["item"], rng.integers(0, In, len(df))], 1).astype(np.int32)
    mats = (sp.coo_matrix((fx["rating"], (fx["user"], fx["item"])), shape=(Un, In)), U.get_inter_matrix(df, _config(fx)))
    outs = []
    for mat in mats:
        torch.manual_seed(0)
        cfg = mf_config(user_num=Un, item_num=In, factors=16, num_layers=2, algo_name=algo, reg_1=0.0, reg_2=0.0, lr=0.01,
                        epochs=1, batch_size=512, inter_matrix=mat, hidden_size_list=[16, 16], node_dropout=0.0,
                        mess_dropout=0.0)
        model = (LightGCN if algo == "lightgcn" else NGCF)(cfg)
        graph = [t.clone() for t in model._adj().coo()]
        model.fit(get_dataloader(BasicDataset(samples), batch_size=512, shuffle=False, num_workers=0))
        outs.append((graph, model.epoch_losses[0]))
    (ga, la), (gb, lb) = outs
    assert all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(ga, gb)) and len(ga[0]) > 0
    assert np.isfinite(la) and np.float64(la).tobytes() == np.float64(lb).tobytes()


# ---- sizes the padded pair cannot or can only just take ------------------------------------------------------------------
def _comb_frame(short_rows, long_len, seed):
    """`short_rows` rows of one entry each and, after them in the frame, one more row of `long_len` distinct columns"""
    rng = np.random.default_rng(seed)
    user = np.concatenate([np.arange(short_rows), np.full(long_len, short_rows)])
    long_cols = rng.permutation(long_len)
    item = np.concatenate([rng.integers(0, long_len, short_rows), long_cols])
    rating = np.concatenate([rng.integers(1, 6, short_rows), rng.integers(1, 6, long_len)]).astype(np.float64)
    order = rng.permutation(len(user))
    order = np.concatenate([order[user[order] != short_rows], np.flatnonzero(user == short_rows)])   # the long row's order kept
    return {"user": user[order], "item": item[order], "rating": rating[order], "user_num": short_rows + 1, "item_num": long_len}


def test_refusal_names_history_csr_and_the_csr_route_serves():
    from daisyrec_amd.utils import utils as U
    fx = _comb_frame(2 ** 20, 2 ** 16, 7)
    df = pd.DataFrame({k: fx[k] for k in ("user", "item", "rating")})
    assert fx["user_num"] * 2 ** 16 * 12 > 800e9                      # 824 GB padded: more than any MI355X holds
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with pytest.raises(MemoryError, match="history_csr"):
        U.get_history_matrix(df, _config(fx), use_config_value_name=True)
    assert torch.cuda.max_memory_allocated() - before < 64 << 20     # the code columns and the counts, never the pair
    row_ptr, col, val, L = U.history_csr(df, _config(fx), use_config_value_name=True)
    want = O.csr_direct(fx["user"], fx["item"], fx["rating"], fx["user_num"], fx["item_num"])
    assert L == 2 ** 16 == want[3]
    assert _same(_host(row_ptr), want[0]) and _same(_host(col), want[1]) and _same(_host(val), want[2])


def test_cell_indices_past_2_31():
    """2^15 + 1 rows, the longest 2^16: 2^31 + 2^16 cells.  The long row is the last one, so its cells and the row before
    it lie past cell 2^31."""
    from daisyrec_amd.utils import utils as U
    short, long_len = 2 ** 15, 2 ** 16
    fx = _comb_frame(short, long_len, 8)
    cells = (short + 1) * long_len
    assert cells == 2 ** 31 + 2 ** 16
    need = cells * 12 + (1 << 30)                                     # the pair plus scratch and the reductions below
    free = torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
    if free < need:
        pytest.skip(f"the device reports {free} free bytes; the [{short + 1}, {long_len}] pair and scratch need {need}")
    df = pd.DataFrame({k: fx[k] for k in ("user", "item", "rating")})
    ids, vals, lens = U.get_history_matrix(df, _config(fx), use_config_value_name=True)
    try:
        assert tuple(ids.shape) == tuple(vals.shape) == (short + 1, long_len) and ids.numel() > 2 ** 31
        is_long = fx["user"] == short
        first_col = np.empty(short + 1, dtype=np.int64)
        first_val = np.empty(short + 1, dtype=np.float32)
        first_col[fx["user"][~is_long]], first_val[fx["user"][~is_long]] = fx["item"][~is_long], fx["rating"][~is_long]
        first_col[short], first_val[short] = fx["item"][is_long][0], fx["rating"][is_long][0]
        # the long (and last) row, whole; every row's first cell; the row before the last
        assert _same(_host(ids[short]), fx["item"][is_long]) and _same(_host(vals[short]), fx["rating"][is_long].astype(np.float32))
        assert _same(_host(ids[:, 0]), first_col) and _same(_host(vals[:, 0]), first_val)
        assert int(ids[short - 1, 0]) == first_col[short - 1] and int(ids[short - 1, 1:].abs().sum()) == 0
        assert float(vals[short - 1, 1:].abs().sum()) == 0.0
        # nothing else anywhere: the device-side sums of both tensors are the frame's
        assert int(ids.sum()) == int(fx["item"].sum())
        assert float(vals.sum(dtype=torch.float64)) == float(fx["rating"].sum())
        assert int(ids.min()) >= 0 and float(vals.min()) >= 0.0
        want_len = np.ones(short + 1, dtype=np.int64)
        want_len[short] = long_len
        assert _same(_host(lens), want_len)
    finally:
        del ids, vals
        gc.collect()
        torch.cuda.empty_cache()
