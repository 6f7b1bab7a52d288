"""iALS / WRMF: weighted matrix factorisation of implicit feedback by alternating least squares, fitted by HIP kernels.

No counterpart in the reference: the model of Hu, Koren and Volinsky (2008) behind the interface of the
fitted models here.  Every cell (u, i) has a preference p_ui (1 where the user interacted, else 0) and a confidence
c_ui = 1 + alpha r_ui; the objective sum_ui c_ui (p_ui - <x_u, y_i>)^2 + reg (|X|^2 + |Y|^2) is minimised exactly in the
user table with the item table fixed (``ops.ials_half_sweep``: per user the normal equations on the fp64 MFMA and a
Cholesky solve in LDS) and then in the item table, ``epochs`` times.  It is the non-sampled counterpart of ``MF`` + BPR:
the same two float32 tables (``embed_user`` / ``embed_item`` are ``nn.Embedding``s) and the same dot-product score, so
``predict`` / ``rank`` / ``full_rank`` / ``full_rank_users`` / ``full_rank_positions`` call exactly what ``MF`` calls.
There is no negative sampler, no learning rate and no CPU path.

``fit(train_set)`` takes the training DataFrame like ``EASE.fit``; duplicate (user, item) pairs are summed.
``fold_in(history)`` gives the factors of users who need not be in training.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from .. import ops
from .. import _native as N
from .AbstractRecommender import GeneralRecommender
from ._frame import frame_columns


class IALS(GeneralRecommender):
    def __init__(self, config):
        """Config keys: factors, reg (> 0), alpha (>= 0), epochs (full sweeps), topk, user_num, item_num, UID_NAME /
        IID_NAME / INTER_NAME (the frame's columns), early_stop, init_method ('default': normal(0, 0.01) from torch's
        global generator, user table first, as MF draws it), gpu, logger."""
        super().__init__(config)
        self.inter_name = config["INTER_NAME"]
        self.iid_name = config["IID_NAME"]
        self.uid_name = config["UID_NAME"]
        self.user_num = int(config["user_num"])
        self.item_num = int(config["item_num"])
        self.factors = int(config["factors"])
        self.reg = float(config["reg"])
        self.alpha = float(config["alpha"])
        self.epochs = int(config["epochs"])
        self.topk = int(config["topk"])
        self.early_stop = bool(config.get("early_stop", False))
        init = config.get("init_method", "default")
        self.initializer = init if init != "default" else "normal"
        if not self.reg > 0 or not math.isfinite(self.reg):
            raise ValueError(f"IALS: reg={self.reg} must be positive and finite (the Gram matrix alone is singular whenever "
                             "the other table has fewer independent rows than factors)")
        if not self.alpha >= 0 or not math.isfinite(self.alpha):
            raise ValueError(f"IALS: alpha={self.alpha} must be >= 0 and finite")
        if self.factors < 1 or self.factors > N.IALS_MAX_D:
            raise ValueError(f"IALS: factors={self.factors} outside [1, {N.IALS_MAX_D}], the systems the kernel holds in LDS")
        if self.epochs < 0:
            raise ValueError(f"IALS: epochs={self.epochs} must be >= 0")
        if self.topk < 1:
            raise ValueError(f"IALS: topk={self.topk} must be >= 1")
        if self.user_num < 1 or self.item_num < 1:
            raise ValueError(f"IALS: user_num={self.user_num}, item_num={self.item_num} must be positive")
        self.embed_user = nn.Embedding(self.user_num, self.factors)
        self.embed_item = nn.Embedding(self.item_num, self.factors)
        self.apply(self._init_weight)
        self.loss_history = []
        self.fit_info = None
        self._is_fitted = False

    # -- fit -----------------------------------------------------------------------------------------------------------
    def _frame_columns(self, df):
        """the configured columns: ids range-checked, ratings finite and >= 0"""
        users, items, ratings = frame_columns(df, (self.uid_name, self.iid_name, self.inter_name), self.user_num,
                                              self.item_num, "IALS")
        if ratings.size and ratings.min() < 0:
            raise ValueError(f"IALS.fit: column '{self.inter_name}' holds a negative value ({ratings.min()}): a confidence "
                             "1 + alpha r below 1 is outside the model")
        return users, items, ratings

    def _tables(self):
        """(P, Q): the weights on the device, contiguous"""
        self._require_device()
        if not self.embed_user.weight.is_cuda:
            self.to(self.device)
        return self.embed_user.weight.data, self.embed_item.weight.data

    def load_state_dict(self, *args, **kw):
        """fitted tables loaded from a checkpoint score like the model that wrote them"""
        out = super().load_state_dict(*args, **kw)
        self._is_fitted = True
        return out

    def fit(self, train_set):
        """`epochs` times: the user half-sweep, the item half-sweep, the objective (one host read per epoch, which also
        brings the two status words).  loss_history lists the objectives; early_stop ends the fit when two successive
        ones differ by less than 1e-5 (the reference's rule, AbstractRecommender.py:131-135)."""
        users, items, ratings = self._frame_columns(train_set)
        P, Q = self._tables()
        dev = P.device
        u, i, r = (torch.from_numpy(a).to(dev) for a in (users, items, ratings))
        csr, csr_t = ops.slim_csr(u, i, r, self.user_num, self.item_num), ops.slim_csr(i, u, r, self.item_num, self.user_num)

        def run_epoch(epoch):
            _, info_u = ops.ials_half_sweep(csr, Q, self.alpha, self.reg, out=P, validate=False)
            _, info_i = ops.ials_half_sweep(csr_t, P, self.alpha, self.reg, out=Q, validate=False)
            loss = ops.ials_objective(csr, P, Q, self.alpha, self.reg)
            loss, bad_u, bad_i = torch.stack([loss, info_u[0].to(torch.float64), info_i[0].to(torch.float64)]).tolist()
            for bad, what in ((bad_u, "user"), (bad_i, "item")):
                if bad != 0:
                    raise RuntimeError(f"IALS.fit: epoch {epoch}: the system of {what} row {int(bad) - 1} is not positive "
                                       f"definite (a Cholesky pivot is not positive; reg={self.reg})")
            return loss, 0

        self._run_epochs(run_epoch, progress=False)
        self.loss_history = list(self.epoch_losses)
        self.fit_info = {"epochs_run": len(self.loss_history), "nnz": int(csr[1].numel()),
                         "bytes_held": sum(t.numel() * t.element_size() for t in (P, Q))}
        self._is_fitted = True

    def _fitted(self):
        self._require_device()
        if not self._is_fitted:
            raise RuntimeError("IALS: fit(train_set) has not been called")
        return self._tables()

    # -- fold-in -------------------------------------------------------------------------------------------------------
    def fold_in(self, history, validate=True):
        """Factors float32 [n, d] (device) of n users from their histories alone - one user half-sweep against the
        fitted item table; the users need not be in training and the model is not touched.  history: a CSR triple
        (row_ptr int64 [n + 1], items int32, ratings float32) on the device, or a dict {row: {item: rating}} with rows
        0 .. n - 1 (a missing row is an empty history).  Ranking the new users, without what they have already seen:

            X_new = model.fold_in(history)
            ids = ops.full_rank_users(X_new, model.embed_item.weight.data, torch.arange(len(X_new)), topk, exclude=history[:2])
        """
        _, Q = self._fitted()
        if isinstance(history, dict):
            n = (max(history) + 1) if history else 0
            rows = [(int(u), int(i), float(r)) for u, row in history.items() for i, r in row.items()]
            if any(u < 0 for u, _, _ in rows):
                raise ValueError("IALS.fold_in: negative row key")
            cols = [torch.tensor([t[k] for t in rows], dtype=dt, device=Q.device)
                    for k, dt in ((0, torch.int64), (1, torch.int64), (2, torch.float64))]
            if rows and (int(cols[1].min()) < 0 or int(cols[1].max()) >= self.item_num):
                raise IndexError(f"IALS.fold_in: item ids must lie in [0, {self.item_num})")
            history = ops.slim_csr(cols[0], cols[1], cols[2], n, self.item_num)
        X, info = ops.ials_half_sweep(history, Q, self.alpha, self.reg, validate=validate)
        bad = int(info.cpu().item())
        if bad != 0:
            raise RuntimeError(f"IALS.fold_in: the system of row {bad - 1} is not positive definite")
        return X

    # -- scores: what MF calls on (P, Q) -------------------------------------------------------------------------------
    def forward(self, user, item):
        P, Q = self._fitted()
        user = torch.as_tensor(user).to(P.device)
        item = torch.as_tensor(item).to(P.device)
        return ops.mf_predict(P, Q, user.reshape(-1), item.reshape(-1)).view(user.shape)

    def predict(self, u, i):
        """<P[u], Q[i]> -> one float"""
        P, Q = self._fitted()
        return float(ops.mf_predict(P, Q, torch.tensor([u], device=P.device), torch.tensor([i], device=P.device)).cpu().item())

    def rank(self, test_loader):
        """float32 [n_users, topk] like MF.rank: the candidates' ids, best first"""
        P, Q = self._fitted()
        return self._rank_loader(test_loader, lambda us, cands_ids: ops.mf_rank_topk(P, Q, us, cands_ids, self.topk))

    def full_rank(self, u):
        """int64 [topk] over all items"""
        P, Q = self._fitted()
        return ops.mf_full_rank(P, Q, int(u), self.topk).cpu().numpy()

    def full_rank_users(self, users, exclude=None, return_scores=False):
        """MF.full_rank_users on the fitted tables"""
        P, Q = self._fitted()
        return self._full_rank_users(P, Q, users, exclude, return_scores)

    def full_rank_positions(self, users, targets, exclude=None, **kw):
        """MF.full_rank_positions on the fitted tables"""
        P, Q = self._fitted()
        return self._full_rank_positions(P, Q, users, targets, exclude, **kw)
