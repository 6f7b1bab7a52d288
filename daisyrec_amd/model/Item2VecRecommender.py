"""Item2Vec recommender with the reference's interface, trained by the MF kernels.

Mirror of daisy/model/Item2VecRecommender.py:15-112: one shared item table, skip-gram pairs
(target, context, label) from `SkipGramNegativeSampler`, BCE-with-logits (sum), Adam by default; after
training the user table is the sum of each user's training items' vectors.  A training step is the
point-wise MF path with P = Q = S (include/daisyrec_amd.h, Item2Vec section); there is no CPU path.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .. import _native as N
from .AbstractRecommender import GeneralRecommender


class Item2Vec(GeneralRecommender):
    def __init__(self, config):
        """Config keys as in Item2VecRecommender.py:29-45: user_num, item_num, factors, lr, epochs, train_ur,
        optimizer, init_method, early_stop, topk, gpu, logger."""
        super().__init__(config)
        self.user_embedding = nn.Embedding(config["user_num"], config["factors"])
        self.ur = config["train_ur"]
        self.shared_embedding = nn.Embedding(config["item_num"], config["factors"])
        self.lr = config["lr"]
        self.epochs = config["epochs"]
        self.loss_type = "CL"                                                     # :38-39
        self.optimizer = config["optimizer"] if config["optimizer"] != "default" else "adam"
        self.initializer = config["init_method"] if config["init_method"] != "default" else "normal"
        self.early_stop = config["early_stop"]
        self.topk = config["topk"]
        self.apply(self._init_weight)

    def _tables(self):
        self._require_device()
        if not self.shared_embedding.weight.is_cuda:
            self.to(self.device)
        return self.user_embedding.weight.data, self.shared_embedding.weight.data

    def forward(self, target_i, context_j):
        """:47-51"""
        _, S = self._tables()
        t = torch.as_tensor(target_i).to(S.device).reshape(-1)
        c = torch.as_tensor(context_j).to(S.device).reshape(-1)
        return ops.mf_predict(S, S, t, c)

    def _step(self, ctx, S, gA, gB, t, c, y):
        """loss into ctx.stats / epoch_acc; d loss / d S into gA (gB is scratch, left zero)."""
        ctx.set_batch(t, c, y)
        ctx.forward(S, S, N.LOSS_CL)
        ctx.stats[1:7] = 0                          # no regulariser in Item2Vec.calc_loss (:61-69)
        ctx.finalize(0.0, 0.0, accumulate=True)
        ctx.item_grad_data(S, S, N.ITEM_CHUNKED, gQ=gB)        # rows of the contexts
        ctx.user_grad(S, S, 0.0, 0.0, gA)                      # rows of the targets
        ops.axpby(gB, 1.0, 1.0, gA, zero_x=True)

    def calc_loss(self, batch):
        """:61-69 (0-dim float64 device tensor; no autograd graph)."""
        _, S = self._tables()
        t, c, y = (torch.as_tensor(x).to(torch.int32).to(S.device).contiguous() for x in batch[:3])
        ctx = ops.BprContext(t.numel(), S.shape[1], S.shape[0], S.shape[0], device=S.device)
        try:
            ctx.set_pointwise(True)
            self._step(ctx, S, torch.zeros_like(S), torch.zeros_like(S), t, c, y)
            return ctx.stats[N.ST_LOSS].clone()
        finally:
            ctx.close()

    def fit(self, train_loader):
        """AbstractRecommender.py:103-137, then the user-embedding build of Item2VecRecommender.py:53-59."""
        opt = self._resolve_optimizer()
        Uemb, S = self._tables()
        triples, n, B = self._train_rows(train_loader)
        gA, gB = torch.zeros_like(S), torch.zeros_like(S)
        optim = ops.DenseOptimizer(opt, self.lr)
        ctx = ops.BprContext(min(B, max(n, 1)), S.shape[1], S.shape[0], S.shape[0], device=S.device)
        ctx.set_pointwise(True)

        def run_epoch(epoch):
            order = self._epoch_rows(train_loader, triples, n)
            ctx.epoch_acc.zero_()
            for s in range(0, n, B):
                rows = order[s:s + B]
                t, c, y = (rows[:, k].contiguous() for k in range(3))
                self._step(ctx, S, gA, gB, t, c, y)
                optim.next_step()
                optim.step(S, gA)          # also clears the gradient
            acc = ctx.epoch_acc.cpu()
            return float(acc[0]), float(acc[1])

        try:
            self._run_epochs(run_epoch)
        finally:
            torch.cuda.synchronize()
            ctx.close()
        self.logger.info("Start building user embedding...")
        users = np.concatenate([np.full(len(v), u, np.int32) for u, v in self.ur.items()]) if self.ur else np.zeros(0, np.int32)
        items = np.concatenate([np.fromiter(v, np.int32, len(v)) for v in self.ur.values()]) if self.ur else np.zeros(0, np.int32)
        if users.size:
            indptr, cols = ops.build_user_csr(torch.from_numpy(users).to(S.device), torch.from_numpy(items).to(S.device),
                                              Uemb.shape[0])
            ops.csr_row_sum(indptr, cols, S, Uemb)

    def predict(self, u, i):
        """:71-80"""
        Uemb, S = self._tables()
        return float(ops.mf_predict(Uemb, S, torch.tensor([u], device=S.device), torch.tensor([i], device=S.device)).cpu().item())

    def rank(self, test_loader):
        """:82-101 -> float32 [n_users, topk]"""
        Uemb, S = self._tables()
        return self._rank_loader(test_loader, lambda us, cands_ids: ops.mf_rank_topk(Uemb, S, us, cands_ids, self.topk))

    def full_rank(self, u):
        """:103-112 -> int64 [topk]"""
        Uemb, S = self._tables()
        return ops.mf_full_rank(Uemb, S, int(u), self.topk).cpu().numpy()

    def full_rank_positions(self, users, targets, exclude=None, **kw):
        """exact ranks of held-out items over the user and item tables (MF.full_rank_positions)"""
        Uemb, S = self._tables()
        return self._full_rank_positions(Uemb, S, users, targets, exclude, **kw)

    def full_rank_users(self, users, exclude=None, return_scores=False):
        """full ranking of many users over the user and item tables (MF.full_rank_users)"""
        Uemb, S = self._tables()
        return self._full_rank_users(Uemb, S, users, exclude, return_scores)
