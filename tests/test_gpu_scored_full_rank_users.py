"""full_rank_users of NeuMF, NFM and VAECF: against the reference's stored full rankings
(tests/golden/kat_neumf.npz, kat_nfm.npz, kat_vae.npz), against tests/full_rank_oracle.py applied to the scores the
existing score entries return, across chunk sizes, and through the KPI frame.  What is promised bit for bit and what per
chunk is DESIGN.md §26's: NFM and NeuMF 'fp32' do not depend on the chunk; the bf16 levels of NeuMF and VAECF are the
exact ranking of the chunk's own scores.  Every test here fails without the feature (NotImplementedError from the base
class)."""
import functools
import logging
import os

import numpy as np
import pytest
import torch

import full_rank_oracle as FO
from conftest import mf_config
from test_oracle_nfm import nfm_config
from test_oracle_vae import vae_config

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("neumf", "nfm", "vae")
U, TOPK = 60, 10
ITEMS = (90, 1100)              # below and above one step of the selector (ops.RANK_ROWS_STEP = 1024)


def _kat(name):
    return np.load(os.path.join(HERE, "golden", f"kat_{name}.npz"))


# ---- the reference's own full rankings ------------------------------------------------------------------------------------
def test_neumf_equals_the_reference_full_ranking():
    from daisyrec_amd.model import NeuMF
    g = _kat("neumf")
    Un, In, d, L = (int(x) for x in g["rank/meta"])
    m = NeuMF(mf_config(user_num=Un, item_num=In, factors=d, num_layers=L, dropout=0.0, model_name="NeuMF", GMF_model=None,
                        MLP_model=None, algo_name="neumf", topk=int(g["rank/topk"])))
    for k, p in m._named().items():
        p.data.copy_(torch.from_numpy(g[f"rank/{k}"]))
    us = g["rank/us"]
    got = m.full_rank_users(us).cpu().numpy()
    own = np.stack([m.full_rank(int(u)) for u in us])
    print("neumf: rows equal to full_rank", (got == own).all(1).sum(), "of", len(us), "; positions equal to rank/full",
          (got == g["rank/full"]).mean())
    assert np.array_equal(got, own)
    assert np.array_equal(got, g["rank/full"])


@pytest.mark.parametrize("bn", [1, 0])
def test_nfm_equals_the_reference_full_ranking(bn):
    from daisyrec_amd.model import NFM
    kat = _kat("nfm")
    Un, In, f, C, nB, topk = (int(x) for x in kat["rank/meta"])
    key = f"rank/bn{bn}_eval"
    m = NFM(nfm_config(user_num=Un, item_num=In, factors=f, num_layers=2, batch_norm=bool(bn), dropout=0.0, topk=topk))
    m.load_state_dict({k: torch.from_numpy(kat[f"{key}/before/p/{k}"].copy()) for k in m.state_dict()})
    m.eval()
    us = kat["rank/us"]
    got = m.full_rank_users(us).cpu().numpy()
    assert np.array_equal(got, kat[f"{key}/full"])
    assert np.array_equal(got, np.stack([m.full_rank(int(u)) for u in us]))


def test_vae_equals_the_reference_full_ranking():
    from daisyrec_amd.model import VAECF
    kat = _kat("vae")
    Un, In, C, nB, topk, lat, ncalls = (int(x) for x in kat["rank/meta"])
    torch.manual_seed(3)
    m = VAECF(vae_config(user_num=Un, item_num=In, mlp_hidden_size=[16], latent_dim=lat, topk=topk,
                         history_item_id=torch.from_numpy(kat["rank/hist_id"]),
                         history_item_value=torch.from_numpy(kat["rank/hist_val"])))
    m.load_state_dict({k[len("rank/params/p/"):]: torch.from_numpy(kat[k]) for k in kat.files
                       if k.startswith("rank/params/p/")})
    m.eval()
    us = kat["rank/us"]
    got = m.full_rank_users(us).cpu().numpy()
    assert np.array_equal(got, kat["rank/eval/full"])
    assert np.array_equal(got, np.stack([m.full_rank(int(u)) for u in us]))


# ---- a small random model ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frame(I):
    """(train_ur, test_ur): about 18 % of U x I seen, a fifth of it held out, every user trains at least one item"""
    rng = np.random.default_rng(31 + I)
    seen = rng.random((U, I)) < 0.18
    seen[np.arange(U), rng.integers(0, I, U)] = True
    u, i = np.nonzero(seen)
    test = rng.random(u.size) < 0.2
    test[np.unique(u, return_index=True)[1]] = False
    train_ur = {int(a): set(i[~test][u[~test] == a].tolist()) for a in range(U)}
    test_ur = {int(a): set(i[test][u[test] == a].tolist()) for a in np.unique(u[test])}
    return train_ur, test_ur


def _history(train_ur, I):
    """the padded pair get_history_matrix would give: ids int64 [U, L] (0 behind a row's end), values 1 / 0"""
    L = max(len(s) for s in train_ur.values())
    hid, hval = np.zeros((U, L), np.int64), np.zeros((U, L), np.float32)
    for a, s in train_ur.items():
        hid[a, :len(s)] = sorted(s)
        hval[a, :len(s)] = 1.0
    return torch.from_numpy(hid), torch.from_numpy(hval)


def _build(name, I, topk=TOPK, **over):
    from daisyrec_amd import model as M
    torch.manual_seed(11)
    if name == "neumf":
        cfg = dict(factors=8, num_layers=2)
        cfg.update(over)
        return M.NeuMF(mf_config(user_num=U, item_num=I, dropout=0.0, model_name="NeuMF", GMF_model=None, MLP_model=None,
                                 algo_name="neumf", topk=topk, **cfg))
    if name == "nfm":
        m = M.NFM(nfm_config(user_num=U, item_num=I, factors=8, num_layers=2, batch_norm=True, dropout=0.5, topk=topk, **over))
        with torch.no_grad():                                   # statistics and biases a fit would have moved
            for bn in m._bn_modules():
                bn.running_mean.normal_(0.0, 0.3)
                bn.running_var.uniform_(0.5, 1.5)
            m.u_bias.weight.normal_(0.0, 0.1)
            m.i_bias.weight.normal_(0.0, 0.1)
        return m.eval()
    hid, hval = _history(_frame(I)[0], I)
    cfg = dict(mlp_hidden_size=[16], latent_dim=8, history_item_id=hid, history_item_value=hval)
    cfg.update(over)
    return M.VAECF(vae_config(user_num=U, item_num=I, topk=topk, **cfg)).eval()


@functools.lru_cache(maxsize=None)
def _model(name, I):
    return _build(name, I)


def _scores(name, m, users):
    """the all-item scores [n, I] the model's EXISTING score entry returns for these users in one call"""
    I = m.embed_item_GMF.num_embeddings if name == "neumf" else (m.embed_item.num_embeddings if name == "nfm" else m.item_num)
    us = torch.as_tensor(np.asarray(users, np.int64)).cuda()
    items = torch.arange(I, device="cuda").repeat(len(users))
    if name == "nfm":
        return m._scores(us, items, C_=I).view(len(users), I).cpu().numpy()
    if name == "neumf":
        ctx = m._ctx(min(len(users) * I, 1 << 18))
        try:
            return ctx.scores(m._params(), us, items, C_=I).view(len(users), I).cpu().numpy()
        finally:
            ctx.close()
    return m._scores(us).cpu().numpy()


def _test_users(I):
    test_ur = _frame(I)[1]
    return list(test_ur)[::-1] + [list(test_ur)[0]]             # unsorted, one user twice


@pytest.mark.parametrize("I", ITEMS)
@pytest.mark.parametrize("name", NAMES)
def test_equals_the_oracle_on_the_models_own_scores(name, I, tmp_path):
    from daisyrec_amd.utils.metrics import calc_ranking_results
    from daisyrec_amd.utils.utils import user_csr
    m = _model(name, I)
    train_ur, test_ur = _frame(I)
    test_u = _test_users(I)
    m.full_rank_users(test_u, exclude=train_ur)                 # (VAECF: sizes the shared score context)
    scores = _scores(name, m, test_u)
    assert scores.shape == (len(test_u), I) and scores.dtype == np.float32
    want_ids, want_sc = FO.rank_lists(scores, FO.exclusion_sets(train_ur, test_u), TOPK)
    preds = m.full_rank_users(test_u, exclude=train_ur)
    assert isinstance(preds, torch.Tensor) and preds.is_cuda and preds.dtype == torch.int64 and preds.shape == (len(test_u), TOPK)
    assert np.array_equal(preds.cpu().numpy(), want_ids)
    pairs = np.array([(a, b) for a in range(U) for b in sorted(train_ur[a])], np.int64)
    ids, sc = m.full_rank_users(np.asarray(test_u), exclude=user_csr(pairs.T, U), return_scores=True)
    assert torch.equal(ids, preds)                              # dict and device CSR: the same exclusion
    sc = sc.cpu().numpy()
    assert sc.dtype == np.float32 and np.array_equal(sc.view(np.uint32), want_sc.view(np.uint32))
    assert not any(set(row.tolist()) & train_ur[a] for row, a in zip(ids.cpu().numpy(), test_u))
    cfg = {"logger": logging.getLogger("full-rank-scored-test"), "res_path": str(tmp_path / "res"), "item_num": I, "topk": TOPK,
           "metrics": ["recall", "mrr", "ndcg", "hit", "precision"]}
    users = list(test_ur)
    got = calc_ranking_results(test_ur, m.full_rank_users(users, exclude=train_ur), users, cfg)
    ref_ids = FO.rank_lists(_scores(name, m, users), FO.exclusion_sets(train_ur, users), TOPK)[0]
    assert got.equals(calc_ranking_results(test_ur, ref_ids, users, cfg))


@pytest.mark.parametrize("name", ["nfm", "neumf"])
def test_rows_equal_full_rank_and_do_not_depend_on_the_chunk(name):
    I = ITEMS[1]
    m = _model(name, I)
    train_ur = _frame(I)[0]
    users = [5, 0, 59, 5, 17, 33, 41]                           # n = 7: the last chunk of two is partial
    plain = m.full_rank_users(users).cpu().numpy()
    for b, u in enumerate(users):
        assert np.array_equal(plain[b], m.full_rank(u)), (name, u)
    assert torch.equal(m.full_rank_users(torch.tensor(users), exclude=None), m.full_rank_users(np.asarray(users)))
    outs = [m.full_rank_users(users, exclude=train_ur, return_scores=True, chunk_bytes=4 * I * r) for r in (1, 2, len(users))]
    outs.append(m.full_rank_users(users, exclude=train_ur, return_scores=True))
    for ids, sc in outs[1:]:
        assert torch.equal(ids, outs[0][0]) and torch.equal(sc.view(torch.int32), outs[0][1].view(torch.int32)), name


def test_vae_chunks_are_the_exact_ranking_of_their_own_scores():
    """mlp_hidden_size = [256]: the GEMMs may split K by the call's row count, so the bits of a score depend on the chunk;
    each chunk's lists are the oracle's on what _scores returns for exactly that chunk's users in the same context"""
    I = ITEMS[1]
    m = _build("vae", I, mlp_hidden_size=[256], latent_dim=64)
    train_ur = _frame(I)[0]
    users = [5, 0, 59, 5, 17, 33, 41]
    m.full_rank_users(users, exclude=train_ur)                  # sizes the shared score context for every call below
    ctx = m._sctx
    for r in (len(users), 2, 1):
        ids, sc = m.full_rank_users(users, exclude=train_ur, return_scores=True, chunk_bytes=4 * I * r)
        ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
        for b0 in range(0, len(users), r):
            chunk = users[b0:b0 + r]
            want_ids, want_sc = FO.rank_lists(m._scores(torch.tensor(chunk)).cpu().numpy(),
                                              FO.exclusion_sets(train_ur, chunk), TOPK)
            assert np.array_equal(ids[b0:b0 + r], want_ids), (r, b0)
            assert np.array_equal(sc[b0:b0 + r].view(np.uint32), want_sc.view(np.uint32)), (r, b0)
    assert m._sctx is ctx


def test_neumf_bf16_storage_keeps_the_invariants():
    """precision 'bf16': whole 128-row tiles of a call run at level 2, so a score's bits depend on the chunk: only what
    holds for every chunk is asserted"""
    I = 1152                                                    # 9 x 128: every chunk is whole tiles, so level 2 runs
    m = _build("neumf", I, factors=64, num_layers=2, precision="bf16")
    train_ur = dict(_frame(I)[0])
    train_ur[3] = set(range(I - 4))                             # four eligible items: a short list
    users = [5, 3, 59, 5, 17, 33, 41]
    for chunk_bytes in (None, 4 * I * 2):
        ids, sc = m.full_rank_users(users, exclude=train_ur, return_scores=True, chunk_bytes=chunk_bytes)
        ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
        for b, u in enumerate(users):
            want = min(TOPK, I - len(train_ur[u]))
            got = ids[b, :want]
            assert np.all(ids[b, want:] == -1) and np.all(np.isneginf(sc[b, want:])), (u, "fill")
            assert np.all((got >= 0) & (got < I)) and len(set(got.tolist())) == want, (u, "ids distinct and in range")
            assert not (set(got.tolist()) & train_ur[u]), (u, "excluded id returned")
            s = sc[b, :want]
            assert np.all(np.isfinite(s)) and np.all(s[1:] <= s[:-1]), (u, "scores rise")
            same = s[1:] == s[:-1]
            assert np.all(got[1:][same] > got[:-1][same]), (u, "equal scores not in ascending id")
        assert sorted(ids[1, :4].tolist()) == [I - 4, I - 3, I - 2, I - 1]


# ---- behaviour --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nfm", "vae"])
def test_training_mode_is_refused_and_nothing_of_the_model_changes(name):
    I = ITEMS[0]
    m = _build(name, I)
    m.train()
    with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):
        m.full_rank_users([1, 2])
    m.eval()
    m.full_rank_users([1, 2])                                   # (moves the parameters to the device)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    calls, update = m._score_calls, getattr(m, "update", None)
    m.full_rank_users([4, 1, 7, 4], exclude=_frame(I)[0], return_scores=True, chunk_bytes=4 * I * 3)
    assert m._score_calls == calls and getattr(m, "update", None) == update
    after = m.state_dict()
    assert list(after) == list(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k


@pytest.mark.parametrize("name", NAMES)
def test_short_lists_and_errors(name, tmp_path):
    from daisyrec_amd import model as M
    from daisyrec_amd.utils.metrics import calc_ranking_results
    I = ITEMS[0]
    m = _model(name, I)
    few = m.full_rank_users([2], exclude={2: set(range(I - 3))}).cpu().numpy()
    assert sorted(few[0, :3].tolist()) == [I - 3, I - 2, I - 1] and np.all(few[0, 3:] == -1)
    cfg = {"logger": logging.getLogger("full-rank-scored-test"), "res_path": str(tmp_path / "res"), "item_num": I, "topk": TOPK,
           "metrics": ["recall", "hit"]}
    with pytest.raises(ValueError, match="pred_ur: item id -1"):
        calc_ranking_results({2: {I - 1}}, few, [2], cfg)
    with pytest.raises(IndexError):
        m.full_rank_users([0, U])
    indptr = np.zeros(U + 1, np.int64)
    indptr[2:] = 2
    with pytest.raises(ValueError, match="ascending"):
        m.full_rank_users([1], exclude=(torch.from_numpy(indptr).cuda(), torch.tensor([9, 3], dtype=torch.int32).cuda()))
    m.topk = 129                                                # (the cutoff of a call, read when it is made)
    try:
        with pytest.raises(ValueError, match="cap of 128"):
            m.full_rank_users([1])
    finally:
        m.topk = TOPK
    assert m.full_rank_users([]).shape == (0, TOPK)
    # what does not change: the base class and MostPop
    with pytest.raises(NotImplementedError, match="full_rank_users"):
        M.AbstractRecommender().full_rank_users([1])
    other = M.MostPop(mf_config(user_num=U, item_num=I, topk=10, algo_name="mostpop"))
    with pytest.raises(NotImplementedError, match="full_rank_users"):
        other.full_rank_users([1])


def test_vae_from_the_history_csr_alone_gives_the_same_lists():
    from daisyrec_amd import ops
    I = ITEMS[1]
    train_ur = _frame(I)[0]
    hid, hval = _history(train_ur, I)
    csr = ops.vae_history_csr(hid.cuda(), hval.cuda(), I)
    padded = _model("vae", I)
    direct = _build("vae", I, history_item_id=None, history_item_value=None, history_csr=csr)
    users = _test_users(I)
    a = padded.full_rank_users(users, exclude=train_ur, return_scores=True)
    b = direct.full_rank_users(users, exclude=train_ur, return_scores=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
