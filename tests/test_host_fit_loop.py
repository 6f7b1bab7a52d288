"""The host plumbing every model shares, without a GPU: the epoch driver, the flat parameter buffer, the rank loop and the
owner of a native handle (GeneralRecommender._run_epochs / ._rank_loader, model/_flat.py, ops._Native)."""
import importlib
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import mf_config


def _model(script, epochs=5, early_stop=False, progress=False):
    """a minimal GeneralRecommender whose run_epoch replays `script` [(loss_sum, nonfinite)] and records what it saw"""
    from daisyrec_amd.model.AbstractRecommender import GeneralRecommender

    class Scripted(GeneralRecommender):
        def run_epoch(self, epoch):
            self.seen.append((epoch, self.training))
            return self.script[epoch - 1]

    m = Scripted(mf_config(progress=progress))
    m.epochs, m.early_stop, m.script, m.seen = epochs, early_stop, list(script), []
    return m


# -- the epoch driver --------------------------------------------------------------------------------------------------
def test_driver_runs_every_epoch_in_training_mode_and_leaves_eval_mode():
    sums = [5.0, 4.0, 3.5, 3.25, 3.0]
    m = _model([(s, 0.0) for s in sums])
    m.epoch_losses = [99.0]                      # (a fit starts from an empty list)
    m._run_epochs(m.run_epoch)
    assert m.seen == [(e, True) for e in range(1, 6)]
    assert m.training is False
    assert m.epoch_losses == sums


def test_driver_stops_early_at_two_equal_sums():
    m = _model([(5.0, 0.0), (4.0, 0.0), (4.0, 0.0), (1.0, 0.0), (0.5, 0.0)], early_stop=True)
    m._run_epochs(m.run_epoch)
    assert m.epoch_losses == [5.0, 4.0, 4.0] and [e for e, _ in m.seen] == [1, 2, 3]
    m = _model([(5.0, 0.0), (4.0, 0.0), (4.0, 0.0), (1.0, 0.0), (0.5, 0.0)], early_stop=False)
    m._run_epochs(m.run_epoch)
    assert len(m.epoch_losses) == 5


def test_driver_stops_after_epoch_one_when_the_first_sum_is_tiny():
    m = _model([(5e-6, 0.0), (4.0, 0.0), (3.0, 0.0), (2.0, 0.0), (1.0, 0.0)], early_stop=True)   # last_loss starts at 0.0
    m._run_epochs(m.run_epoch)
    assert m.epoch_losses == [5e-6] and m.training is False


@pytest.mark.parametrize("bad", [(math.nan, 0.0), (math.inf, 0.0), (-math.inf, 0.0), (1.0, 1.0)])
def test_driver_raises_the_reference_error_on_a_non_finite_epoch(bad):
    m = _model([(5.0, 0.0), (4.0, 0.0), bad, (2.0, 0.0), (1.0, 0.0)])
    with pytest.raises(ValueError, match="Loss=Nan or Infinity"):
        m._run_epochs(m.run_epoch)
    assert m.epoch_losses == [5.0, 4.0]
    assert [e for e, _ in m.seen] == [1, 2, 3]


def test_driver_writes_the_epoch_log(tmp_path, monkeypatch):
    log = tmp_path / "epochs.log"
    monkeypatch.setenv("DAISY_AMD_EPOCH_LOG", str(log))
    sums = [5.0, 0.1 + 0.2, 4.0, 4.0, 1.0]
    m = _model([(s, 0.0) for s in sums], early_stop=True)
    m._run_epochs(m.run_epoch)
    assert log.read_text().splitlines() == [f"Scripted epoch {e} loss {s!r}" for e, s in enumerate(sums[:4], 1)]


def test_driver_builds_a_bar_only_when_asked(monkeypatch):
    A = importlib.import_module("daisyrec_amd.model.AbstractRecommender")      # (the package exports the class by this name)
    bars = []

    class Bar:
        def __init__(self, it):
            self.it, self.desc, self.post = it, [], []
            bars.append(self)

        def __iter__(self):
            return iter(self.it)

        def set_description(self, text):
            self.desc.append(text)

        def set_postfix(self, **kw):
            self.post.append(kw)

    monkeypatch.setattr(A, "_tqdm", Bar)
    script = [(3.0, 0.0), (2.0, 0.0)]
    m = _model(script, epochs=2, progress=False)            # config['progress'] = False
    m._run_epochs(m.run_epoch)
    m = _model(script, epochs=2, progress=True)
    m._run_epochs(m.run_epoch, progress=False)              # the sharded fit: no bar per rank
    assert bars == []
    m._run_epochs(m.run_epoch)
    assert len(bars) == 1 and bars[0].desc == ["[Epoch 001]", "[Epoch 002]"] and bars[0].post == [{"loss": 3.0}, {"loss": 2.0}]
    monkeypatch.setattr(A, "_tqdm", None)                   # tqdm not installed
    m._run_epochs(m.run_epoch)
    assert m.epoch_losses == [3.0, 2.0]


# -- the flat parameter buffer -----------------------------------------------------------------------------------------
def _net():
    torch.manual_seed(7)
    return nn.Sequential(nn.Linear(5, 3), nn.Tanh(), nn.Linear(3, 2))


def test_flatten_keeps_the_state_dict_and_aliases_every_parameter():
    from daisyrec_amd.model._flat import flatten_parameters, views_live, views_of
    net = _net()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    flat = flatten_parameters(net.named_parameters(), "cpu", transposed=("0.weight",))
    assert flat.shape == (15 + 3 + 6 + 2,) and flat.dtype == torch.float32
    after = net.state_dict()
    assert list(after) == list(before)
    for k in before:
        assert after[k].shape == before[k].shape and torch.equal(after[k], before[k]), k
    assert torch.equal(flat[:15].view(5, 3), before["0.weight"].t())       # stored transposed: input-major
    assert torch.equal(flat[15:18], before["0.bias"]) and torch.equal(flat[18:24].view(2, 3), before["2.weight"])
    assert views_live(flat, net.parameters())
    flat.add_(1.0)                                                         # the optimiser's pass over the buffer
    for k in before:
        assert torch.equal(net.state_dict()[k], before[k] + 1.0), k
    g = views_of(torch.zeros_like(flat), net.named_parameters())
    assert {k: tuple(v.shape) for k, v in g.items()} == {k: tuple(v.shape) for k, v in before.items()}


def test_views_live_tells_a_rehomed_module_from_a_loaded_one():
    from daisyrec_amd.model._flat import flatten_parameters, views_live
    net = _net()
    assert not views_live(None, net.parameters())
    flat = flatten_parameters(net.named_parameters(), "cpu", transposed=("0.weight",))
    other = {k: v + 0.5 for k, v in _net().state_dict().items()}
    net.load_state_dict(other)                                            # copies in place: the views stay
    assert views_live(flat, net.parameters())
    assert torch.equal(flat[:15].view(5, 3), other["0.weight"].t())
    net.double().float()                                                  # every p.data re-homed, as by .cpu() / .cuda()
    assert all(p.device == flat.device and p.dtype == flat.dtype for p in net.parameters())
    assert not views_live(flat, net.parameters())
    old = flat.clone()
    flat.add_(1.0)
    assert torch.equal(net.state_dict()["2.bias"], other["2.bias"])       # ... and the buffer no longer reaches them
    assert torch.equal(flat, old + 1.0)
    flat2 = flatten_parameters(net.named_parameters(), "cpu", transposed=("0.weight",))
    assert views_live(flat2, net.parameters()) and not views_live(flat, net.parameters())
    assert torch.equal(flat2, old)                                        # the current values, not the stale buffer's
    assert not views_live(flat2, list(net.parameters())[::-1])            # (another order is another layout)


# -- the rank loop -----------------------------------------------------------------------------------------------------
def test_rank_loader_on_the_host():
    m = _model([])
    m.device = "cpu"
    seen = []

    def topk_of(us, cands_ids):
        seen.append((us.clone(), cands_ids.clone()))
        return cands_ids[:, :2].to(torch.int64)

    empty = m._rank_loader([], topk_of)
    assert empty.shape == (0,) and empty.dtype == np.float32 and seen == []
    batches = [(torch.tensor([[3], [4]]), torch.tensor([[7, 8, 9], [1, 2, 3]])),      # users [Bu, 1] -> [Bu]
               (torch.tensor(5), torch.tensor([6, 5, 4]))]                            # one user, a 1-D candidate row
    out = m._rank_loader(batches, topk_of)
    assert out.dtype == np.float32 and np.array_equal(out, np.array([[7, 8], [1, 2], [6, 5]], np.float32))
    assert [tuple(u.shape) for u, _ in seen] == [(2,), (1,)]
    assert [tuple(c.shape) for _, c in seen] == [(2, 3), (1, 3)]
    assert torch.equal(seen[1][1], torch.tensor([[6, 5, 4]]))


# -- the owner of a native handle --------------------------------------------------------------------------------------
def test_native_handle_is_destroyed_once_and_a_failed_constructor_is_harmless():
    import ctypes as C
    from daisyrec_amd import ops
    calls = []

    def destroy(h):
        calls.append(h.value)
        return 0

    class Owner(ops._Native):
        _destroy = destroy
        _bytes = staticmethod(lambda h: 40 + h.value)

        def __init__(self, fail=False):
            if fail:
                raise RuntimeError("before the handle was set")
            self._h = C.c_void_p(2)

    o = Owner()
    assert o.nbytes == 42
    o.close()
    o.close()
    assert calls == [2] and not o._h.value
    o.__del__()
    assert calls == [2]
    broken = Owner.__new__(Owner)
    with pytest.raises(RuntimeError):
        broken.__init__(fail=True)
    broken.close()
    broken.__del__()
    assert calls == [2]

    def failing(h):
        raise OSError("library gone")

    class Late(Owner):
        _destroy = failing

    Late().__del__()                                                      # __del__ never raises
    for cls in (ops.TrainIndex, ops.EpochPlan, ops.BprContext, ops.LgcnGraph, ops.NeumfContext, ops.NfmContext,
                ops.VaeContext):
        assert issubclass(cls, ops._Native) and cls._destroy is not None and cls._bytes is not None
    assert isinstance(ops.BprContext.scratch_bytes, property)
