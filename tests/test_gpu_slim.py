"""SLiM on the device (csrc/slim.hip) against the numpy oracle (tests/slim_oracle.py) and the reference's golden vectors:
the Gram matrix (exact with integer ratings, across user blocks, bitwise repeatable), the coordinate descent fed the same
G (supports, values, sweep counts; both state placements), the scores, and the model end to end through
SLiM.fit(DataFrame)."""
import functools

import numpy as np
import pytest
import torch

import slim_oracle as O
from test_oracle_slim import RULES, TAGS, case, oracle_fit, oracle_ranks, slim_config

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _csr(u, i, r, U, I):
    from daisyrec_amd import ops
    return ops.slim_csr(torch.as_tensor(np.array(u)).to(DEV), torch.as_tensor(np.array(i)).to(DEV),
                        torch.as_tensor(np.array(r, dtype=np.float64)).to(DEV), U, I)


@functools.lru_cache(None)
def device_gram(tag):
    from daisyrec_amd import ops
    c = case(tag)
    return ops.slim_gram(_csr(c["u"], c["i"], c["r"], c["U"], c["I"]), c["I"])


def _columns(count, rows, vals):
    count, rows, vals = count.cpu().numpy(), rows.cpu().numpy(), vals.cpu().numpy()
    for j in range(len(count)):                       # unused slots are (-1, 0)
        assert (rows[j, count[j]:] == -1).all() and (vals[j, count[j]:] == 0).all()
    return [(rows[j, :count[j]], vals[j, :count[j]]) for j in range(len(count))]


def _dense_w(cols, I):
    W = np.zeros((I, I), np.float32)
    for j, (rows, vals) in enumerate(cols):
        W[rows, j] = vals
    return W


# ---- Gram --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_gram_is_exact_with_integer_ratings(tag):
    G = device_gram(tag).cpu().numpy()
    assert G.dtype == np.float32 and np.array_equal(G.astype(np.float64), case(tag)["G"])


def _real_case():
    U, I = 200, 130
    u, i, _ = O.fixture(U, I, .08, 7, True)
    r = np.random.RandomState(7).uniform(0.5, 5.0, len(u)).astype(np.float32)
    return U, I, u, i, r


def test_gram_real_ratings_within_the_fp32_accumulation_bound():
    from daisyrec_amd import ops
    U, I, u, i, r = _real_case()
    G = ops.slim_gram(_csr(u, i, r, U, I), I).cpu().numpy().astype(np.float64)
    want = O.gram(O.dense(u, i, r.astype(np.float64), U, I))
    rel = np.abs(G - want).max() / np.abs(want).max()
    elem = (np.abs(G - want) / np.where(want == 0, 1.0, np.abs(want))).max()
    print(f"max |G - G64| / max |G64| = {rel:.3e}; largest element-wise relative error {elem:.3e}")
    assert np.array_equal(G == 0, want == 0)
    assert (np.abs(G - want) <= 1e-6 * np.abs(want)).all()


def test_gram_accumulates_across_user_blocks():
    from daisyrec_amd import ops
    c = case("B")                                      # 200 users through a 64-row tile: four blocks, the last one short
    G = ops.slim_gram(_csr(c["u"], c["i"], c["r"], c["U"], c["I"]), c["I"], tile_rows=64).cpu().numpy()
    assert np.array_equal(G.astype(np.float64), c["G"])
    U, I, u, i, r = _real_case()
    csr = _csr(u, i, r, U, I)
    G1, G2 = ops.slim_gram(csr, I, tile_rows=48), ops.slim_gram(csr, I, tile_rows=48)
    assert torch.equal(G1, G2)                         # bitwise, run to run
    want = O.gram(O.dense(u, i, r.astype(np.float64), U, I))
    assert (np.abs(G1.cpu().numpy() - want) <= 1e-6 * np.abs(want)).all()


def test_gram_refuses_what_does_not_fit():
    from daisyrec_amd import ops
    c = case("A")
    with pytest.raises(ValueError, match="does not fit the 4096 bytes offered"):
        ops.slim_gram(_csr(c["u"], c["i"], c["r"], c["U"], c["I"]), c["I"], offered_bytes=4096)


# ---- coordinate descent ------------------------------------------------------------------------------------------------
def _check_against_oracle(tag, rule, path):
    from daisyrec_amd import ops
    c = case(tag)
    tol, max_iter = RULES[rule]
    count, rows, vals, sweeps, gap = ops.slim_fit(device_gram(tag), c["U"], c["alpha"], c["elastic"], c["topk"], tol=tol,
                                                  max_iter=max_iter, path=path)
    cols = _columns(count, rows, vals)
    _, o_sweeps, o_gaps, o_kept, _ = oracle_fit(tag, rule)
    yy = np.diag(c["G"])
    worst = 0.0
    for j, ((r_d, v_d), (r_o, v_o)) in enumerate(zip(cols, o_kept)):
        assert np.array_equal(r_d, r_o), (tag, rule, j)                 # same support, same order
        if len(v_o):
            worst = max(worst, np.abs(v_d.astype(np.float64) - v_o.astype(np.float64)).max())
    print(f"{tag} {rule} {path}: max |w - w_oracle| over the kept entries = {worst:.3e}; sweeps {o_sweeps.min()}..{o_sweeps.max()}")
    assert worst <= 1e-9
    rated = yy > 0
    assert np.array_equal(sweeps.cpu().numpy()[rated], o_sweeps[rated])
    assert (count.cpu().numpy()[~rated] == 0).all()
    # the gap's five sums run in another order: terms of the size of yy, a few hundred of them, in fp64
    assert (np.abs(gap.cpu().numpy() - o_gaps) <= 1e-9 * np.maximum(yy, 1.0)).all()
    return count, rows, vals, sweeps, gap


@pytest.mark.parametrize("rule", sorted(RULES))
@pytest.mark.parametrize("tag", TAGS)
def test_descent_equals_the_sequential_oracle(tag, rule):
    _check_against_oracle(tag, rule, "auto")


@pytest.mark.parametrize("tag", TAGS)
def test_descent_with_the_state_in_global_memory(tag):
    from daisyrec_amd import ops
    c = case(tag)
    got = _check_against_oracle(tag, "default", "global")
    lds = ops.slim_fit(device_gram(tag), c["U"], c["alpha"], c["elastic"], c["topk"], path="lds")
    for a, b in zip(got, lds):
        assert torch.equal(a, b)


def test_descent_column_ranges_and_l1_only():
    from daisyrec_amd import ops
    c = case("B")
    G = device_gram("B")
    whole = ops.slim_fit(G, c["U"], c["alpha"], c["elastic"], c["topk"])
    part = ops.slim_fit(G, c["U"], c["alpha"], c["elastic"], c["topk"], col0=37, ncols=21)
    for a, b in zip(whole, part):
        assert torch.equal(a[37:58], b)
    # l1_ratio = 1 (b = 0) is legal
    count, rows, vals, sweeps, gap = ops.slim_fit(G, c["U"], 0.05, 1.0, c["topk"], col0=0, ncols=4)
    for j, (r_d, v_d) in enumerate(_columns(count, rows, vals)):
        w, s, _ = O.cd_column(c["G"], j, c["U"], 0.05, 1.0)
        r_o, v_o = O.truncate(w, c["topk"])
        assert np.array_equal(r_d, r_o) and np.abs(v_d.astype(np.float64) - v_o).max() <= 1e-9 and int(sweeps[j]) == s


def test_descent_switches_to_global_state_above_the_lds_limit():
    """item_num just above the LDS limit, 64 users, the 8 most rated items moved to the last 8 columns: the automatic
    path is the global-state kernel; its 8 columns against the oracle on the device's own G"""
    from daisyrec_amd import _native as N
    from daisyrec_amd import ops
    U, I = 64, N.SLIM_LDS_ITEMS + 16
    u, i, r = O.fixture(U, I, .002, 11, False)
    cnt = np.bincount(i, minlength=I)
    top = np.argsort(-cnt, kind="stable")[:8]
    perm = np.arange(I)
    for t, dst in zip(top, range(I - 8, I)):
        a, b = np.nonzero(perm == t)[0][0], dst
        perm[[a, b]] = perm[[b, a]]                    # perm[new id] = old id
    inv = np.empty(I, np.int64)
    inv[perm] = np.arange(I)
    i = inv[i]
    assert np.bincount(i, minlength=I)[I - 8:].min() >= 2
    G = ops.slim_gram(_csr(u, i, r, U, I), I)
    alpha, l1r, topk = 0.02, 0.3, 6
    count, rows, vals, sweeps, gap = ops.slim_fit(G, U, alpha, l1r, topk, col0=I - 8, ncols=8)
    Gh = G.cpu().numpy()
    assert np.array_equal(Gh[I - 8:, I - 8:].astype(np.float64), O.gram(O.dense(u, i, r, U, I)[:, I - 8:]))
    kept = 0
    for n, (r_d, v_d) in enumerate(_columns(count, rows, vals)):
        w, s, g = O.cd_column(Gh, I - 8 + n, U, alpha, l1r)
        r_o, v_o = O.truncate(w, topk)
        assert np.array_equal(r_d, r_o) and int(sweeps[n]) == s
        if len(r_o):
            assert np.abs(v_d.astype(np.float64) - v_o).max() <= 1e-9
        kept += len(r_o)
    assert kept >= 8
    with pytest.raises(ValueError, match="LDS path"):
        ops.slim_fit(G, U, alpha, l1r, topk, col0=I - 8, ncols=8, path="lds")


# ---- scores ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["lds", "global"])
def test_scores_equal_the_oracle_bit_for_bit(path):
    from daisyrec_amd import ops
    c = case("B")
    W, _, _, kept, _ = oracle_fit("B")
    count = torch.tensor([len(r) for r, _ in kept], dtype=torch.int32, device=DEV)
    rows = torch.full((c["I"], c["topk"]), -1, dtype=torch.int32)
    vals = torch.zeros((c["I"], c["topk"]), dtype=torch.float32)
    for j, (r_, v_) in enumerate(kept):
        rows[j, :len(r_)] = torch.from_numpy(r_)
        vals[j, :len(r_)] = torch.from_numpy(v_)
    Wd = ops.slim_columns(count, rows.to(DEV), vals.to(DEV), c["I"])
    with pytest.raises(ValueError, match="item_num"):
        ops.slim_columns(count[:7], rows[:7].to(DEV), vals[:7].to(DEV), c["I"])
    csr = _csr(c["u"], c["i"], c["r"], c["U"], c["I"])
    users = torch.arange(c["U"], device=DEV)
    got = ops.slim_scores(csr, Wd, c["I"], users, torch.from_numpy(c["cands"].copy()).to(DEV), path=path).cpu().numpy()
    assert np.array_equal(got, oracle_ranks("B")[0])
    some = np.array([3, 0, 199, 3, 77])
    full = ops.slim_scores(csr, Wd, c["I"], torch.from_numpy(some).to(DEV), path=path).cpu().numpy()
    assert np.array_equal(full, O.scores(c["X"], W, some))


# ---- the model ---------------------------------------------------------------------------------------------------------
def _frame(u, i, r):
    import pandas as pd
    return pd.DataFrame({"user": np.asarray(u), "item": np.asarray(i), "rating": np.asarray(r, dtype=np.float64)})


@functools.lru_cache(None)
def fitted(tag):
    from daisyrec_amd.model import SLiM
    c = case(tag)
    m = SLiM(slim_config(alpha=c["alpha"], elastic=c["elastic"], topk=c["topk"], user_num=c["U"], item_num=c["I"]))
    m.fit(_frame(c["u"], c["i"], c["r"]), verbose=False)
    return m


def _loader(c, batch=64):
    cands = torch.from_numpy(c["cands"].copy())
    return [(torch.arange(u0, min(u0 + batch, c["U"])), cands[u0:u0 + batch]) for u0 in range(0, c["U"], batch)]


@pytest.mark.parametrize("tag", TAGS)
def test_fit_against_the_reference_and_the_oracle(tag):
    import scipy.sparse as sp
    c = case(tag)
    m = fitted(tag)
    ws = m.w_sparse
    assert sp.isspmatrix_csr(ws) and ws.dtype == np.float32 and ws.shape == (c["I"], c["I"])
    W = np.asarray(ws.todense())
    assert np.array_equal(W != 0, c["W_ref"] != 0)
    dist = np.abs(W.astype(np.float64) - c["W_ref"].astype(np.float64)).max()
    print(f"{tag}: max |W - W_ref| = {dist:.3e}, bound {c['ref_dist'] + c['oracle_dist'] + 1e-9:.3e}")
    assert dist <= c["ref_dist"] + c["oracle_dist"] + 1e-9
    assert np.abs(W.astype(np.float64) - oracle_fit(tag)[0]).max() <= 1e-9
    assert set(m.fit_info) == {"sweeps", "gap"} and m.fit_info["sweeps"].shape == (c["I"],)
    assert np.array_equal(m.fit_info["sweeps"][np.diag(c["G"]) > 0], oracle_fit(tag)[1][np.diag(c["G"]) > 0])

    ranks = m.rank(_loader(c))
    k = min(c["topk"], c["cands"].shape[1])
    assert ranks.shape == (c["U"], k) and ranks.dtype == np.int64
    assert np.array_equal(ranks, oracle_ranks(tag)[1])            # the oracle's lists, from its own truncated float32 W
    agree = (ranks == c["rank_ref"]).mean()
    print(f"{tag}: rank positions equal to the reference's: {agree:.4%}")
    assert agree >= 0.99


def test_predict_full_rank_and_a_tilde_are_consistent_with_rank():
    c = case("C")
    m = fitted("C")
    A = m.A_tilde
    assert A.shape == (c["U"], c["I"]) and A.dtype == np.float64
    W = np.asarray(m.w_sparse.todense())
    assert np.array_equal(A.astype(np.float32), O.scores(c["X"], W, np.arange(c["U"])))
    for u in (0, 17, c["U"] - 1):
        fr = m.full_rank(u)
        assert fr.dtype == np.int64 and np.array_equal(fr, np.argsort(-A[u], kind="stable")[:c["topk"]])
        for it in c["cands"][u, :3]:
            p = m.predict(u, int(it))
            assert isinstance(p, float) and p == A[u, it]
    ranks = m.rank(_loader(c, batch=50))
    want = O.rank_lists(np.take_along_axis(A, c["cands"], 1).astype(np.float32), c["cands"], c["topk"])
    assert np.array_equal(ranks, want)
    with pytest.raises(IndexError):
        m.predict(c["U"], 0)
    with pytest.raises(IndexError):
        m.predict(0, c["I"])


def test_duplicate_rows_are_summed_and_fits_repeat_bitwise():
    from daisyrec_amd.model import SLiM
    c = case("C")
    u, i, r = c["u"], c["i"], c["r"]
    split = r >= 2                                     # every rating >= 2 arrives as two rows (1, r - 1), far apart
    frame = _frame(np.concatenate([u, u[split]]), np.concatenate([i, i[split]]),
                   np.concatenate([np.where(split, 1.0, r), r[split] - 1.0]))
    cfg = slim_config(alpha=c["alpha"], elastic=c["elastic"], topk=c["topk"], user_num=c["U"], item_num=c["I"])
    a, b = SLiM(cfg), SLiM(dict(cfg, slim_slab_bytes=8 * c["topk"] * 128))      # b: three column chunks (128, 128, 44)
    a.fit(frame, verbose=False)
    b.fit(_frame(u, i, r), verbose=False)              # a second fit of the same data: the column queue is dynamic
    assert b.slab_bytes // (8 * c["topk"]) == 128 < c["I"]
    ref = fitted("C")
    for x in (a, b):
        for t0, t1 in zip(x._W, ref._W):
            assert torch.equal(t0, t1)
        assert torch.equal(x._csr[2], ref._csr[2]) and torch.equal(x._csr[1], ref._csr[1])
    assert np.array_equal(a.fit_info["gap"], ref.fit_info["gap"]) and np.array_equal(b.fit_info["sweeps"], ref.fit_info["sweeps"])
