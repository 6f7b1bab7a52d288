"""model.fit_many without a device: every refusal names the model and the reason before a device is asked for, the
native entry point rejects bad arguments without a HIP call, the epoch rule exists once, and the exact cases of
tests/test_gpu_fit_many.py lie in the exact domain of tests/segment_layouts.py."""
import ctypes
import inspect
import logging

import pytest
import torch

import fit_many_cases as F
from daisyrec_amd.model import FM, MF, fit_many
from daisyrec_amd.model.AbstractRecommender import GeneralRecommender
from daisyrec_amd.utils.dataset import BasicDataset, get_dataloader


def _config(**over):
    cfg = {"gpu": "0", "logger": logging.getLogger("t"), "lr": 0.05, "reg_1": 0.001, "reg_2": 0.002, "epochs": 2, "topk": 10,
           "user_num": F.U, "item_num": F.I, "factors": 32, "loss_type": "BPR", "optimizer": "sgd", "init_method": "default",
           "early_stop": False, "progress": False, "seed": 7, "shuffle_mode": "device"}
    cfg.update(over)
    return cfg


def _model(cls=MF, **over):
    m = cls(_config(**over))
    m.device = "cpu"              # whatever this machine has: a model that passes the checks must then ask for a device
    return m


def _loader(batch_size=256, shuffle=True, n=F.N_TRIPLES):
    return get_dataloader(BasicDataset(F.triples(n)), batch_size=batch_size, shuffle=shuffle, num_workers=0)


def test_an_empty_list_returns_an_empty_list():
    assert fit_many([], _loader()) == []
    assert fit_many([], []) == []


def test_eligible_models_reach_the_device_check():
    with pytest.raises(RuntimeError, match="no HIP device"):
        fit_many([_model(), _model(factors=64, loss_type="HL")], _loader())
    with pytest.raises(RuntimeError, match="no HIP device"):
        fit_many([_model(shuffle_mode="loader")], _loader(shuffle=False))        # a SequentialSampler draws no order


REFUSED = [
    (lambda: _model(FM), {}, "FM is not MF"),
    (lambda: _model(optimizer="adam"), {}, "optimizer 'adam'"),
    (lambda: _model(optimizer="no-such-optimizer"), {}, "optimizer 'adam'"),       # the reference's fallback
    (lambda: _model(loss_type="CL"), {}, "loss_type 'CL' is point-wise"),
    (lambda: _model(loss_type="SL"), {}, "loss_type 'SL' is point-wise"),
    (lambda: _model(item_mode="sorted"), {}, "item_mode 'sorted'"),
    (lambda: _model(item_mode="atomic"), {}, "item_mode 'atomic'"),
    (lambda: _model(), dict(batch_size=257), "batch_size 257 > 256"),
    (lambda: _model(factors=256, row_pitch=0), {}, "do not fit the LDS"),
    (lambda: _model(shuffle_mode="loader"), {}, "shuffle_mode"),
]


@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_refusals_name_the_model_and_the_reason_before_the_device(k):
    make, loader_kw, reason = REFUSED[k]
    good, bad = _model(), make()
    with pytest.raises(ValueError) as err:
        fit_many([good, bad], [_loader(), _loader(**loader_kw)])
    assert "fit_many: model 1: " in str(err.value) and reason in str(err.value), str(err.value)
    assert good.epoch_losses == [] and good.training                  # nothing was touched


def test_a_sharded_fit_and_a_wrong_loader_count_are_refused(monkeypatch):
    bad = _model()
    monkeypatch.setattr(bad, "_sharded_world", lambda: 2)
    with pytest.raises(ValueError, match="fit_many: model 0: .*sharded"):
        fit_many([bad], _loader())
    with pytest.raises(ValueError, match="2 train loaders for 1 models"):
        fit_many([_model()], [_loader(), _loader()])


def test_a_small_training_set_counts_with_its_own_size():
    """min(B, n) decides, as in fit: 100 rows under batch_size 1024 are one batch of 100"""
    with pytest.raises(RuntimeError, match="no HIP device"):
        fit_many([_model()], _loader(batch_size=1024, n=100))


def test_an_unknown_loss_raises_what_fit_raises():
    with pytest.raises(NotImplementedError, match="Invalid loss type"):
        fit_many([_model(loss_type="nope")], _loader())


def test_the_native_entry_rejects_bad_arguments_without_a_hip_call():
    from daisyrec_amd import _native as N
    assert N.lib.daisy_bpr_fit_epoch_sgd_many(None, 1, None, 0, None) == N.DAISY_ERR_ARG
    assert "trials is NULL" in N.last_error()
    assert N.lib.daisy_bpr_fit_epoch_sgd_many(None, -1, None, 0, None) == N.DAISY_ERR_ARG
    assert N.lib.daisy_bpr_fit_epoch_sgd_many(None, 0, None, 0, None) == N.DAISY_OK
    rec = (N.SmallTrial * 2)()                                         # all fields NULL: refused at trial 0, by name
    assert N.lib.daisy_bpr_fit_epoch_sgd_many(rec, 2, None, 0, None) == N.DAISY_ERR_ARG
    assert "trial 0: NULL argument" in N.last_error()
    assert ctypes.sizeof(N.SmallTrial) == 80


def test_the_epoch_rule_exists_once():
    """_run_epochs and fit_many both end an epoch through GeneralRecommender._close_epoch"""
    import daisyrec_amd.model._many as many
    assert "_close_epoch(" in inspect.getsource(GeneralRecommender._run_epochs)
    assert "_close_epoch(" in inspect.getsource(many.fit_many)
    for src in (inspect.getsource(GeneralRecommender._run_epochs), inspect.getsource(many)):
        assert "Loss=Nan" not in src and "1e-5" not in src and "DAISY_AMD_EPOCH_LOG" not in src
    m = _model(early_stop=True)
    m.train()
    assert m._close_epoch(1, 3.0, 0.0, 0.0) is False and m.epoch_losses == [3.0] and not m.training
    assert m._close_epoch(2, 3.0 + 5e-6, 0.0, 3.0) is True and len(m.epoch_losses) == 2
    m.early_stop = False
    assert m._close_epoch(3, 3.0, 0.0, 3.0) is False
    for loss, nonfinite in ((float("nan"), 0.0), (float("inf"), 0.0), (1.0, 1.0)):
        with pytest.raises(ValueError, match="Loss=Nan or Infinity: current settings does not fit the recommender"):
            m._close_epoch(4, loss, nonfinite, 3.0)
    assert len(m.epoch_losses) == 3


def test_the_exact_cases_lie_in_the_exact_domain():
    """every step of the int64 chain passes assert_exact_domain (ExactCase.chain asserts it), the tables stay integers
    that fp32 holds, and the chain does move the tables"""
    tri = F.triples()
    for c in F.exact_cases():
        c.chain(tri)
        assert int(c.P.abs().max()) < 1 << 12 and int(c.Q.abs().max()) < 1 << 12 and c.loss > 0
        assert not torch.equal(c.P.to(torch.float32), torch.from_numpy(c.P0))
