"""model.fit_many / ops.fit_epoch_sgd_many: many small-batch MF models per launch, one workgroup each
(csrc/bpr_small.hip, k_small_epoch_many).  The many-kernel runs the body of the one-model kernel on the same plan, in the
same order, with a single owner per row: every comparison here is torch.equal / == on floats, against `fit`, against
`ctx.fit_epoch_sgd`, and against the int64 restatement of tests/segment_layouts.py."""
import logging

import numpy as np
import pytest
import torch

import fit_many_cases as F
from daisyrec_amd import ops
from daisyrec_amd.model import MF, fit_many
from daisyrec_amd.model.MFRecommender import padded_factors
from daisyrec_amd.utils.dataset import BasicDataset, get_dataloader

pytestmark = pytest.mark.gpu
DEV = "cuda"
NONFINITE = "Loss=Nan or Infinity: current settings does not fit the recommender"


def _config(**over):
    cfg = {"gpu": "0", "logger": logging.getLogger("t"), "lr": 0.05, "reg_1": 0.001, "reg_2": 0.002, "epochs": 3, "topk": 10,
           "user_num": F.U, "item_num": F.I, "factors": 32, "loss_type": "BPR", "optimizer": "sgd", "init_method": "default",
           "early_stop": False, "progress": False, "seed": 7, "shuffle_mode": "device"}
    cfg.update(over)
    return cfg


def _build(specs, seed0=1000):
    """one MF per spec (a dict of config overrides), model k initialised from torch.manual_seed(seed0 + k)"""
    out = []
    for k, spec in enumerate(specs):
        torch.manual_seed(seed0 + k)
        out.append(MF(_config(**spec)))
    return out


def _state(m):
    P, Q = m._tables()                       # the padded buffers where the model trains on a row pitch
    return P.clone(), Q.clone(), list(m.epoch_losses)


def _same(a, b, what):
    (Pa, Qa, la), (Pb, Qb, lb) = _state(a), _state(b)
    assert Pa.shape == Pb.shape and torch.equal(Pa, Pb), f"{what}: P differs"
    assert Qa.shape == Qb.shape and torch.equal(Qa, Qb), f"{what}: Q differs"
    assert la == lb, f"{what}: epoch losses {la} != {lb}"


@pytest.fixture(scope="module")
def loaders():
    tri = F.triples()
    ds = BasicDataset(tri)
    return {"tri": tri,
            "shuffled": get_dataloader(ds, batch_size=256, shuffle=True, num_workers=0),
            "sequential": get_dataloader(ds, batch_size=256, shuffle=False, num_workers=0),
            "shuffled100": get_dataloader(ds, batch_size=100, shuffle=True, num_workers=0),
            "sequential128": get_dataloader(ds, batch_size=128, shuffle=False, num_workers=0)}


# (config overrides, loader, expected (trained columns, dpad, staging mode)) - the table of the design section
TRIALS = [
    (dict(factors=32, loss_type="BPR"), "shuffled", (32, 36, 3)),
    (dict(factors=64, loss_type="HL", reg_1=0.0, reg_2=0.0, lr=0.03), "shuffled", (64, 64, 2)),      # shares trial 0's plan
    (dict(factors=100, row_pitch="auto", loss_type="TL", lr=0.02, seed=8), "shuffled", (128, 128, 1)),
    (dict(factors=128, reg_1=0.002, reg_2=0.001, lr=0.04, seed=9), "sequential", (128, 128, 1)),
    (dict(factors=20, row_pitch=0, loss_type="HL", epochs=1), "sequential", (20, 20, 3)),
    (dict(factors=50, row_pitch=0, reg_1=0.0, reg_2=0.0, lr=0.06, epochs=5), "shuffled", (50, 52, 2)),
    (dict(factors=32, loss_type="TL", seed=10), "shuffled100", (32, 36, 3)),
    (dict(factors=64, lr=0.01, seed=11), "sequential128", (64, 68, 3)),
]


def _dpad_mode(d, B):
    """small_dpad and the staging rule of csrc/bpr_small.hip (kSmallLdsRows = 128 KiB), restated"""
    p = (d + 3) // 4 * 4
    dpad = p + 4 if (p % 32 == 0 and 3 * B * (p + 4) * 4 <= 128 * 1024) else p
    row = B * dpad * 4
    return dpad, 3 if 3 * row <= 128 * 1024 else (2 if 2 * row <= 128 * 1024 else 1)


def test_equal_to_fit_over_every_staging_mode_and_lane_layout(loaders):
    specs = [t[0] for t in TRIALS]
    lds = [loaders[t[1]] for t in TRIALS]
    tri_dev = torch.from_numpy(loaders["tri"]).to(DEV)
    for (spec, name, (dtrain, dpad, mode)), ld in zip(TRIALS, lds):
        B = ld.batch_size
        assert padded_factors(spec["factors"], spec.get("row_pitch", "auto"), B) == dtrain
        assert _dpad_mode(dtrain, B) == (dpad, mode), (spec, _dpad_mode(dtrain, B))
        ctx, plan = ops.BprContext(B, dtrain, F.U, F.I), ops.EpochPlan(F.N_TRIPLES, F.U, F.I)
        plan.build(tri_dev, B)
        assert ops.LazyAdam.small_epoch_supported(ctx, plan, ops.LOSS_IDS[spec.get("loss_type", "BPR")]), spec
        ctx.close(); plan.close()
    alone, many = _build(specs), _build(specs)
    for m, ld in zip(alone, lds):
        m.fit(ld)
    out = fit_many(many, lds)
    assert out == [None] * len(specs)
    for k, (a, b) in enumerate(zip(alone, many)):
        _same(a, b, f"trial {k} {specs[k]}")
        assert len(b.epoch_losses) == specs[k].get("epochs", 3) and not b.training
        assert b.row_pitch == a.row_pitch
    assert many[0].epoch_losses != many[1].epoch_losses


def test_equal_to_the_exact_integer_chain(loaders):
    """the exact domain of tests/segment_layouts.py: the tables after one identity-order epoch are the int64 chain's"""
    cases = [c.chain(loaders["tri"]) for c in F.exact_cases()]
    models = _build([dict(factors=c.d, row_pitch=c.pitch, loss_type="HL", reg_1=0.0, reg_2=0.0, lr=F.EXACT_LR, epochs=1)
                     for c in cases])
    for m, c in zip(models, cases):
        m.embed_user.weight.data.copy_(torch.from_numpy(c.P0))
        m.embed_item.weight.data.copy_(torch.from_numpy(c.Q0))
    assert fit_many(models, loaders["sequential"]) == [None] * len(cases)
    for m, c in zip(models, cases):
        assert torch.equal(m.embed_user.weight.data.cpu(), c.P.to(torch.float32)), f"d={c.d}: P"
        assert torch.equal(m.embed_item.weight.data.cpu(), c.Q.to(torch.float32)), f"d={c.d}: Q"
        assert m.epoch_losses == [float(c.loss)], (c.d, m.epoch_losses, c.loss)


def test_more_workgroups_than_compute_units():
    count = torch.cuda.get_device_properties(0).multi_processor_count + 3
    tri = F.triples(n=64, users=16, items=16, seed=5)
    ld = get_dataloader(BasicDataset(tri), batch_size=32, shuffle=True, num_workers=0)
    spec = lambda k: dict(user_num=16, item_num=16, factors=32, epochs=2, lr=0.01 + 0.0001 * k, seed=7 + k % 3)   # noqa: E731
    many = _build([spec(k) for k in range(count)])
    assert fit_many(many, ld) == [None] * count
    picked = sorted(set(list(range(0, count, max(1, count // 8)))[:8] + [count - 1]))
    for k in picked:
        torch.manual_seed(1000 + k)
        a = MF(_config(**spec(k)))
        a.fit(ld)
        _same(a, many[k], f"model {k} of {count}")


def test_early_stop_leaves_the_launch_and_the_others_train_on(loaders):
    specs = [dict(), dict(lr=0.0, early_stop=True, epochs=4), dict(factors=64, loss_type="HL")]
    alone, many = _build(specs), _build(specs)
    ld = loaders["sequential"]
    for m in alone:
        m.fit(ld)
    assert fit_many(many, ld) == [None] * 3
    assert len(many[1].epoch_losses) == 2 and len(many[0].epoch_losses) == 3 and len(many[2].epoch_losses) == 3
    for k, (a, b) in enumerate(zip(alone, many)):
        _same(a, b, f"model {k}")


def test_a_non_finite_loss_stops_one_model_only(loaders):
    """a NaN / infinite step loss ends that model's epoch on the device before the step's update (the kernel leaves its
    loop); fit raises for it, fit_many hands the same error back in its place"""
    specs = [dict(), dict(factors=64), dict(loss_type="TL")]
    alone, many = _build(specs), _build(specs)
    ld = loaders["sequential"]
    u0 = int(loaders["tri"][0, 0])
    for group in (alone, many):
        group[1].embed_user.weight.data[u0, 0] = float("inf")
    alone[0].fit(ld)
    alone[2].fit(ld)
    with pytest.raises(ValueError, match="Loss=Nan or Infinity"):
        alone[1].fit(ld)
    out = fit_many(many, ld)
    assert out[0] is None and out[2] is None
    assert isinstance(out[1], ValueError) and str(out[1]) == NONFINITE
    for k, (a, b) in enumerate(zip(alone, many)):
        _same(a, b, f"model {k}")
    assert many[1].epoch_losses == [] and not many[1].training


def _ops_world(tri_dev, d, B, seed, plan=None):
    g = torch.Generator().manual_seed(seed)
    P = (torch.randn(F.U, d, generator=g) * 0.1).to(DEV)
    Q = (torch.randn(F.I, d, generator=g) * 0.1).to(DEV)
    if plan is None:
        plan = ops.EpochPlan(F.N_TRIPLES, F.U, F.I).build(tri_dev, B, order="feistel", seed=seed, epoch=1)
    return ops.BprContext(B, d, F.U, F.I), plan, P, Q


def test_ops_level_equals_fit_epoch_sgd_and_refuses_bad_trials(loaders):
    tri_dev = torch.from_numpy(loaders["tri"]).to(DEV)
    a = _ops_world(tri_dev, 32, 256, 1)
    b = _ops_world(tri_dev, 64, 256, 2, plan=a[1])               # shares a's plan
    c = _ops_world(tri_dev, 52, 100, 3)
    hyper = [(0.05, 1e-3, 2e-3, ops.LOSS_IDS["BPR"], 1e-10), (0.02, 0.0, 0.0, ops.LOSS_IDS["HL"], 1e-10),
             (0.03, 2e-3, 1e-3, ops.LOSS_IDS["TL"], 1e-10)]
    worlds = [a, b, c]
    want = []
    for (ctx, plan, P, Q), (lr, r1, r2, lid, gamma) in zip(worlds, hyper):
        ctx2, P2, Q2 = ops.BprContext(ctx.max_batch, ctx.d, F.U, F.I), P.clone(), Q.clone()
        sl = torch.zeros(plan.num_batches, dtype=torch.float64, device=DEV)
        ctx2.fit_epoch_sgd(plan, P2, Q2, lr, r1, r2, loss_type=lid, gamma=gamma, item_mode=ops.ITEM_MODES["fused"], step_losses=sl)
        torch.cuda.synchronize()
        want.append((P2, Q2, sl, ctx2.stats.clone(), ctx2.epoch_acc.clone()))
        ctx2.close()
    sls = [torch.zeros(w[1].num_batches, dtype=torch.float64, device=DEV) for w in worlds]
    ops.fit_epoch_sgd_many([w + h for w, h in zip(worlds, hyper)], step_losses=sls)
    torch.cuda.synchronize()
    for k, ((ctx, plan, P, Q), sl, (P2, Q2, sl2, stats2, acc2)) in enumerate(zip(worlds, sls, want)):
        assert torch.equal(P, P2) and torch.equal(Q, Q2), k
        assert torch.equal(sl, sl2) and float(sl.abs().min()) > 0.0, k
        assert torch.equal(ctx.stats, stats2) and torch.equal(ctx.epoch_acc, acc2), k
    # nothing is launched for a refused call: the tables keep their bits
    before = [w[2].clone() for w in worlds]
    ctx_x = ops.BprContext(256, 32, F.U, F.I)
    with pytest.raises(ValueError, match="trial 1 shares"):
        ops.fit_epoch_sgd_many([a + hyper[0], (ctx_x, a[1], a[2], torch.zeros_like(a[3])) + hyper[0]])
    index = ops.TrainIndex(tri_dev, F.U, F.I)
    part = ops.EpochPlan(F.N_TRIPLES, F.U, F.I).build_indexed(index, 256, order="feistel", seed=1, epoch=1)
    with pytest.raises(ValueError, match="trial 1: not a small-batch epoch"):
        ops.fit_epoch_sgd_many([a + hyper[0], (ctx_x, part, b[2][:, :32].contiguous(), b[3][:, :32].contiguous()) + hyper[0]])
    ops.fit_epoch_sgd_many([])
    torch.cuda.synchronize()
    for w, P0 in zip(worlds, before):
        assert torch.equal(w[2], P0)
    for x in (ctx_x, index, part, a[1], c[1], a[0], b[0], c[0]):
        x.close()


def test_two_calls_from_the_same_start_are_bit_equal(loaders):
    specs = [dict(), dict(factors=100, loss_type="TL", seed=3), dict(factors=50, row_pitch=0, loss_type="HL")]
    first, second = _build(specs), _build(specs)
    assert fit_many(first, loaders["shuffled"]) == [None] * 3 and fit_many(second, loaders["shuffled"]) == [None] * 3
    for k, (a, b) in enumerate(zip(first, second)):
        _same(a, b, f"model {k}")
