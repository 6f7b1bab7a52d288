"""fit_many: the fits of a search trained side by side.

`MF` at the reference's defaults (SGD, a pairwise loss, batch_size 256) trains every step of an epoch inside ONE persistent
workgroup (csrc/bpr_small.hip): one compute unit of the device works, the others idle.  The fits a tuning run asks for -
the trials of a grid over lr / reg / factors, the folds of a cross-validation - are independent models of a few hundred KB:
`fit_many(models, train_loaders)` runs one epoch of ALL of them per native call, one workgroup per model
(ops.fit_epoch_sgd_many), and reads all their epoch losses back in one transfer.  Every model ends with the bits `fit`
gives it: same plan, same kernel body, same order of every sum.
"""
from __future__ import annotations

import torch
from torch.utils.data import SequentialSampler

from .. import ops
from .MFRecommender import MF, padded_factors

PAIRWISE = (ops.N.LOSS_BPR, ops.N.LOSS_HL, ops.N.LOSS_TL)


def _rows_and_batch(loader):
    """(n, B) of a fit over `loader`, on the host (GeneralRecommender._train_rows without the upload)"""
    data = getattr(loader.dataset, "data", None)
    if data is None:
        raise TypeError("fit expects a DataLoader over BasicDataset (dataset.data = int32 [N,3] triples)")
    n, B = int(len(data)), int(loader.batch_size)
    if loader.drop_last:
        n = (n // B) * B
    return n, B


def _refusal(model, loader):
    """why `model` over `loader` cannot join a fit_many call (None: it can) - no device is touched"""
    if type(model) is not MF:
        return (f"{type(model).__name__} is not MF (FM trains biases, the other models have kernels of their own): "
                "call its fit")
    opt = model._resolve_optimizer()
    if opt != "sgd":
        return (f"optimizer {opt!r}: only SGD epochs are independent of every other workgroup (the lazy Adam epoch waits "
                "for helper workgroups); call fit")
    loss_id = model._build_criterion(model.loss_type)
    if loss_id not in PAIRWISE:
        return f"loss_type {model.loss_type!r} is point-wise: the small-batch epoch kernel trains BPR, HL and TL"
    if model.item_mode not in ("fused", "chunked"):
        return f"item_mode {model.item_mode!r}: the small-batch epoch kernel runs under 'fused' and 'chunked' only"
    if model._sharded_world() != 1:
        return "the fit is sharded over the ranks of torch.distributed (config['shard_users']): call fit"
    n, B = _rows_and_batch(loader)
    Bn = min(B, n)
    if Bn > ops.SMALL_BATCH_MAX:
        return f"batch_size {Bn} > {ops.SMALL_BATCH_MAX}: larger batches fill the device by themselves, call fit"
    d = padded_factors(int(model.embed_user.weight.shape[1]), model.row_pitch, Bn if n else None)
    if Bn * ((d + 3) // 4 * 4) * 4 > ops.SMALL_LDS_ROW_BYTES:
        return f"{Bn} rows of {d} factors do not fit the LDS of the small-batch epoch kernel: call fit"
    if not isinstance(loader.sampler, SequentialSampler) and model.shuffle_mode != "device":
        return ("shuffle_mode 'loader' with a shuffled loader replays the global torch RNG, which epochs trained side by "
                "side cannot draw from in the order a sequence of fit calls does: set config['shuffle_mode'] = 'device' "
                "or use a loader without shuffling")
    return None


def fit_many(models, train_loaders):
    """Train `models` (MF, SGD, pairwise loss, batches of at most 256 rows) as `m.fit(loader)` would train each of them,
    all of them side by side: one native call and one host read-back per epoch for all models still running.
    train_loaders: one DataLoader for all models, or a list with one per model (models that share a loader object, its
    batch size, their seed and table sizes share one epoch plan).

    -> a list with one entry per model: None where it trained; the ValueError `fit` would have raised where a step's loss
    was not finite - that model's tables are what `fit` leaves, the others train on.  A model that cannot take this path
    raises ValueError (its index and the reason) before anything is trained."""
    models = list(models)
    if isinstance(train_loaders, (list, tuple)):
        loaders = list(train_loaders)
        if len(loaders) != len(models):
            raise ValueError(f"fit_many: {len(loaders)} train loaders for {len(models)} models")
    else:
        loaders = [train_loaders] * len(models)
    for k, (m, ld) in enumerate(zip(models, loaders)):
        why = _refusal(m, ld)
        if why is not None:
            raise ValueError(f"fit_many: model {k}: {why}")
    if not models:
        return []
    for m in models:
        m._require_device()

    results = [None] * len(models)
    pitches = [getattr(m, "row_pitch", None) for m in models]
    rows = {}            # id(loader) -> (device triples, n, B, user_sorted)
    plans = {}           # (id(loader), n, B, seed, U, I) -> EpochPlan
    fits = {}            # model index -> (ctx, plan key, P, Q, loss id, loader): the models that train at all
    try:
        for k, (m, ld) in enumerate(zip(models, loaders)):
            m.to(m.device)
            loss_id = m._build_criterion(m.loss_type)
            if id(ld) not in rows:
                triples, n, B = m._train_rows(ld)
                rows[id(ld)] = (triples, n, B, ops.triples_user_sorted(triples[:n]) if n else True)
            triples, n, B, _ = rows[id(ld)]
            m.epoch_losses = []
            if n == 0:          # an empty loader: every epoch's loss is 0.0 (GeneralRecommender._fit)
                for _ in range(m.epochs):
                    m.epoch_losses.append(0.0)
                    if m.early_stop:
                        m.logger.info("Satisfy early stop mechanism")
                        break
                continue
            B = min(B, n)
            P, Q = m._tables(batch=B)
            key = (id(ld), n, B, m.seed, P.shape[0], Q.shape[0])
            if key not in plans:
                plans[key] = ops.EpochPlan(n, P.shape[0], Q.shape[0], device=P.device)
            fits[k] = (ops.BprContext(B, P.shape[1], P.shape[0], Q.shape[0], device=P.device), key, P, Q, loss_id, ld)
        models[0].logger.info("HIP fit_many: %d models (%d of them train), %d epoch plan(s): small-batch epoch kernel, one "
                              "workgroup per model", len(models), len(fits), len(plans))

        running = [k for k in fits if models[k].epochs >= 1]
        last_loss = dict.fromkeys(running, 0.0)
        epoch = 1
        while running:
            for key in dict.fromkeys(fits[k][1] for k in running):      # the epoch laid out once per group of models
                triples, n, B, user_sorted = rows[key[0]]
                ld = next(fits[k][5] for k in running if fits[k][1] == key)
                order = "identity" if isinstance(ld.sampler, SequentialSampler) else "feistel"
                plans[key].build(triples, key[2], order=order, seed=key[3], epoch=epoch, n_triples=n, user_sorted=user_sorted)
            trials = []
            for k in running:
                m = models[k]
                ctx, key, P, Q, loss_id, ld = fits[k]
                m.train()
                if isinstance(ld.sampler, SequentialSampler):
                    m._epoch_order(ld, rows[id(ld)][0].shape[0])        # (the draw of one pass over the loader, as in fit)
                trials.append((ctx, plans[key], P, Q, m.lr, m.reg_1, m.reg_2, loss_id, 1e-10))
            accs = [t[0].epoch_acc for t in trials]
            torch._foreach_zero_(accs)
            ops.fit_epoch_sgd_many(trials)
            host = torch.stack(accs).cpu()                               # the one host sync of the epoch, for all models
            still = []
            for x, k in enumerate(running):
                m = models[k]
                loss = float(host[x, 0])
                try:
                    done = m._close_epoch(epoch, loss, float(host[x, 1]), last_loss[k])
                except ValueError as err:
                    results[k] = err
                    continue
                last_loss[k] = loss
                if not done and epoch < m.epochs:
                    still.append(k)
            running = still
            epoch += 1
    finally:
        if fits or rows:
            torch.cuda.synchronize()
        for ctx, *_ in fits.values():
            ctx.close()
        for plan in plans.values():
            plan.close()
        for m, pitch in zip(models, pitches):
            m.eval()
            if pitch is not None:
                m.row_pitch = pitch
    return results
