"""NFM recommender with the reference's interface, trained by HIP kernels.

Mirror of daisy/model/NFMRecommender.py:15-209 (class ``NFM``): same config keys, the same ``nn`` modules built in
the same order (so a seed gives the reference's initial parameters, and ``state_dict`` keys - BatchNorm's
``running_mean`` / ``running_var`` / ``num_batches_tracked`` included - match), same attributes and methods.
``fit`` / ``calc_loss`` / ``rank`` / ``full_rank`` / ``predict`` run through ``daisy_nfm_*`` (include/daisyrec_amd.h,
csrc/nfm.hip): the gather, every Linear / BatchNorm / activation / dropout stage, the criterion and the backward pass,
then one dense optimiser pass over the flat parameter buffer.  There is no CPU path.

As in the reference, a pairwise loss forwards the positives and the negatives as two calls: BatchNorm takes separate
batch statistics for each and updates its running statistics twice per step.  Dropout (nfm.yaml: 0.5) uses the
device's counter-hash masks, not torch's generator: the same distribution, a different stream.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from .. import _native as N
from ._flat import flatten_parameters, views_live, views_of
from .AbstractRecommender import GeneralRecommender


class NFM(GeneralRecommender):
    def __init__(self, config):
        """Config keys as in NFMRecommender.py:16-93."""
        super().__init__(config)
        self.factors = config["factors"]
        self.act_function = config["act_function"]
        self.num_layers = config["num_layers"]
        self.batch_norm = config["batch_norm"]
        self.dropout = config["dropout"]

        self.lr = config["lr"]
        self.reg_1 = config["reg_1"]
        self.reg_2 = config["reg_2"]
        self.epochs = config["epochs"]

        self.loss_type = config["loss_type"]
        self.initializer = config["init_method"] if config["init_method"] != "default" else "xavier_normal"
        self.optimizer = config["optimizer"] if config["optimizer"] != "default" else "sgd"
        self.early_stop = config["early_stop"]
        self.topk = config["topk"]

        d, L = int(self.factors), int(self.num_layers)
        if not (1 <= d <= N.NFM_MAX_FACTORS) or not (0 <= L <= N.NFM_MAX_LAYERS):
            raise ValueError(f"NFM: factors={d} (1..{N.NFM_MAX_FACTORS}), num_layers={L} (0..{N.NFM_MAX_LAYERS}) unsupported")

        self.embed_user = nn.Embedding(config["user_num"], config["factors"])
        self.embed_item = nn.Embedding(config["item_num"], config["factors"])

        self.u_bias = nn.Embedding(config["user_num"], 1)
        self.i_bias = nn.Embedding(config["item_num"], 1)

        self.bias_ = nn.Parameter(torch.tensor([0.0]))

        FM_modules = []
        if self.batch_norm:
            FM_modules.append(nn.BatchNorm1d(config["factors"]))
        FM_modules.append(nn.Dropout(self.dropout))
        self.FM_layers = nn.Sequential(*FM_modules)

        MLP_modules = []
        in_dim = config["factors"]
        for _ in range(self.num_layers):                                  # NFMRecommender.py:70-87
            out_dim = in_dim
            MLP_modules.append(nn.Linear(in_dim, out_dim))
            in_dim = out_dim
            if self.batch_norm:
                MLP_modules.append(nn.BatchNorm1d(out_dim))
            if self.act_function == "relu":
                MLP_modules.append(nn.ReLU())
            elif self.act_function == "sigmoid":
                MLP_modules.append(nn.Sigmoid())
            elif self.act_function == "tanh":
                MLP_modules.append(nn.Tanh())
            MLP_modules.append(nn.Dropout(self.dropout))
        self.deep_layers = nn.Sequential(*MLP_modules)
        predict_size = config["factors"]

        self.prediction = nn.Linear(predict_size, 1, bias=False)

        self._init_weight()
        self._act = self.act_function if self.act_function in ("relu", "sigmoid", "tanh") else "none"
        # knob of the native path (absent from the reference config): 'auto' (default: the layered step), 'small' (the
        # one-workgroup step, batches <= 256) or 'layered' - the same arithmetic and the same bits
        self.step_path = str(config.get("step_path", "auto")).lower()
        if self.step_path not in N.NFM_PATHS:
            raise ValueError(f"config['step_path'] must be one of {sorted(N.NFM_PATHS)}, got {self.step_path!r}")
        self._flat = None
        self._sctx = None
        self._steps = 0           # optimiser steps taken: the dropout key of step k is (seed << 32) | k
        self._score_calls = 0

    def _init_weight(self):
        """NFMRecommender.py:95-108: only the Linear weights are re-initialised (biases keep torch's default)."""
        init = self.initializer_config[self.initializer]
        kw = self.initializer_param_config[self.initializer]
        init(self.embed_user.weight, **kw)
        init(self.embed_item.weight, **kw)
        nn.init.constant_(self.u_bias.weight, 0.0)
        nn.init.constant_(self.i_bias.weight, 0.0)
        if self.num_layers > 0:
            for m in self.deep_layers:
                if isinstance(m, nn.Linear):
                    init(m.weight, **kw)
            init(self.prediction.weight, **kw)
        else:
            nn.init.constant_(self.prediction.weight, 1.0)

    # -- parameters as the kernels see them: ONE flat device buffer, the module's tensors are views ------------------
    def _bn_modules(self):
        """BatchNorm1d of stage 0 (FM_layers) and of every deep layer, in stage order ([] without batch_norm)."""
        if not self.batch_norm:
            return []
        return [self.FM_layers[0]] + [m for m in self.deep_layers if isinstance(m, nn.BatchNorm1d)]

    def _table(self, t):
        """name -> tensor (parameters, or their gradient views) -> the keys of ops._nfm_table."""
        out = {"P": t["embed_user.weight"], "Q": t["embed_item.weight"], "ub": t["u_bias.weight"],
               "ib": t["i_bias.weight"], "bias": t["bias_"], "wp": t["prediction.weight"]}
        lin = [n for n, m in self.deep_layers.named_children() if isinstance(m, nn.Linear)]
        for l, n in enumerate(lin, 1):
            out[f"W{l}"], out[f"b{l}"] = t[f"deep_layers.{n}.weight"], t[f"deep_layers.{n}.bias"]
        if self.batch_norm:
            names = ["FM_layers.0"] + [f"deep_layers.{n}" for n, m in self.deep_layers.named_children()
                                       if isinstance(m, nn.BatchNorm1d)]
            for s, n in enumerate(names):
                out[f"bn_w{s}"], out[f"bn_b{s}"] = t[f"{n}.weight"], t[f"{n}.bias"]
        return out

    def _params(self):
        """Move the parameters into one contiguous device buffer (once), the BatchNorm buffers to the device; returns
        the kernel table of the parameters."""
        self._require_device()
        if not views_live(self._flat, self.parameters()):
            self._flat = flatten_parameters(self.named_parameters(), self.device)
        for m in self._bn_modules():
            for b in ("running_mean", "running_var", "num_batches_tracked"):
                if not getattr(m, b).is_cuda:
                    setattr(m, b, getattr(m, b).to(self.device))
        return self._table(dict(self.named_parameters()))

    def _grad_table(self, gflat):
        return self._table(views_of(gflat, self.named_parameters()))

    def _bn(self):
        mods = self._bn_modules()
        return [(m.running_mean, m.running_var, m.num_batches_tracked) for m in mods] if mods else None

    def _ctx(self, rows):
        ctx = ops.NfmContext(max(int(rows), 1), self.factors, self.num_layers, self._act, self.batch_norm,
                             self.embed_user.num_embeddings, self.embed_item.num_embeddings, device=self.device)
        ctx.set_path(self.step_path)
        return ctx

    def _one_row_check(self, rows):
        if self.batch_norm and self.training and rows == 1:
            raise ValueError("Expected more than 1 value per channel when training, got input size "
                             f"torch.Size([1, {self.factors}])")

    def _check_ids(self, users, items):
        U, I = self.embed_user.num_embeddings, self.embed_item.num_embeddings
        for ids, n, what in ((users, U, "user"), (items, I, "item")):
            if ids is not None and ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= n):
                raise IndexError(f"index out of range in self ({what} id outside 0..{n - 1})")

    def _score_ctx(self, rows):
        """The scoring context, kept on the module: eval mode needs no workspace (one row's), training mode one for
        `rows` pairs (grown when a call scores more)."""
        train = bool(self.training)
        need = max(int(rows), 1) if train else 1
        ctx = getattr(self, "_sctx", None)
        if ctx is None or ctx.max_rows < need:
            if ctx is not None:
                ctx.close()
            ctx = self._sctx = self._ctx(need)
        return ctx

    def _scores(self, users, items=None, C_=0, n=None):
        """NFM.forward over pairs in the module's mode (training mode: batch statistics over all pairs, one running
        statistics update, dropout)."""
        p = self._params()
        rows = int(items.numel()) if items is not None else int(n)
        self._one_row_check(rows)
        train = bool(self.training)
        ctx = self._score_ctx(rows)
        self._score_calls += 1
        return ctx.scores(p, self._bn(), users, items, C_=C_, n=n, train=train, dropout=self.dropout if train else 0.0,
                          seed=self._seed_hi | (0x80000000 + self._score_calls))

    # -- reference surface -------------------------------------------------------------------------------------------
    def forward(self, user, item):
        """NFMRecommender.py:110-123 -> pred [n]."""
        user = torch.as_tensor(user).to(self.device)
        item = torch.as_tensor(item).to(self.device)
        if self.batch_norm and user.dim() == 0:
            raise ValueError("expected 2D or 3D input (got 1D input)")
        user, item = user.reshape(-1), item.reshape(-1)
        self._check_ids(user, item)
        return self._scores(user, item)

    def calc_loss(self, batch):
        """NFMRecommender.py:125-151: the batch loss (0-dim float64 device tensor, no autograd graph, no parameter
        change; like the reference's forward calls it updates the BatchNorm running statistics).  Dropout uses the key
        of the next optimiser step."""
        loss_id = self._build_criterion(self.loss_type)
        p = self._params()
        u, i, j = (torch.as_tensor(x).to(torch.int32).to(self.device).contiguous() for x in batch[:3])
        self._check_ids(u, i if loss_id in ops.POINTWISE_LOSSES else torch.cat([i, j]))
        self._one_row_check(int(u.numel()))
        ctx = self._ctx(u.numel())
        try:
            gflat = torch.zeros_like(self._flat)
            ctx.step_grads(p, self._grad_table(gflat), self._bn(), u, i, j, loss_id, self.reg_1, self.reg_2,
                           dropout=self.dropout if self.training else 0.0, seed=self._seed_hi | (self._steps + 1))
            return ctx.stats[N.NFST_LOSS].clone()
        finally:
            ctx.close()

    def fit(self, train_loader):
        """AbstractRecommender.py:103-137 for NFM: the epoch's steps (daisy_nfm_step_grads + the dense optimiser) are
        issued by the library in one call; one host sync per epoch."""
        opt = self._resolve_optimizer()
        loss_id = self._build_criterion(self.loss_type)
        p = self._params()
        triples, n, B = self._train_rows(train_loader)
        if n > 0:
            pw = loss_id in ops.POINTWISE_LOSSES
            self._check_ids(triples[:n, 0], triples[:n, 1] if pw else triples[:n, 1:3].reshape(-1))
        # the reference's BatchNorm refuses a training batch of one row: it trains the batches before it, then raises
        one_row_tail = bool(self.batch_norm) and n % B == 1
        gflat = torch.zeros_like(self._flat)
        grads = self._grad_table(gflat)
        optim = ops.DenseOptimizer(opt, self.lr)         # a fresh optimiser per fit, as the reference builds one
        ctx = self._ctx(min(B, max(n, 1)))

        def run_epoch(epoch):
            order = self._epoch_rows(train_loader, triples, n)
            cols = [order[:, k].contiguous() for k in range(3)]
            ctx.stats.zero_()
            m = n - 1 if one_row_tail else n
            if m > 0:
                self._steps += ctx.fit_epoch(p, grads, self._bn(), cols[0], cols[1], cols[2], B, optim, self._flat,
                                             gflat, loss_id, self.reg_1, self.reg_2, dropout=self.dropout,
                                             seed_hi=self._seed_hi, step0=self._steps)
            if one_row_tail:
                torch.cuda.synchronize()
                self._one_row_check(1)
            st = ctx.stats.cpu()
            return float(st[N.NFST_LOSS_SUM]), float(st[N.NFST_NONFINITE])

        try:
            self._run_epochs(run_epoch)
        finally:
            torch.cuda.synchronize()
            ctx.close()

    def predict(self, u, i):
        """NFMRecommender.py:153-158 (with batch_norm the reference's BatchNorm1d refuses the 1-D input)."""
        if self.batch_norm:
            raise ValueError("expected 2D or 3D input (got 1D input)")
        return float(self.forward(torch.tensor([u]), torch.tensor([i])).cpu().item())

    def rank(self, test_loader):
        """NFMRecommender.py:160-192 -> float32 [n_users, topk] like the reference."""
        self._params()

        def topk_of(us, cands_ids):
            Bu, C = cands_ids.shape
            self._check_ids(us, cands_ids)
            scores = self._scores(us, cands_ids.reshape(-1), C_=C)
            return ops.topk_from_scores(scores.view(Bu, C), cands_ids, self.topk)

        return self._rank_loader(test_loader, topk_of)

    def full_rank(self, u):
        """NFMRecommender.py:194-209 -> int64 [topk]."""
        self._params()
        I = self.embed_item.num_embeddings
        users = torch.tensor([int(u)], device=self.device)
        self._check_ids(users, None)
        scores = self._scores(users, None, C_=0, n=I)
        return ops.full_topk_from_scores(scores, self.topk).cpu().numpy()

    def full_rank_users(self, users, exclude=None, return_scores=False, chunk_bytes=None, validate=True):
        """Full ranking of many users (no counterpart in the reference): device int64 [len(users),
        min(topk, I)], row b = full_rank(users[b]) without the items of the user's row of `exclude` (None, an (indptr,
        items) device CSR or a train_ur dict of sets); -1 where a user has fewer eligible items than topk.  return_scores:
        (ids, float32 scores).  Eval mode only - batch statistics and dropout over an arbitrary chunk are not a ranking:
        call model.eval() first.  chunk_bytes (default 256 MiB) of scores at a time through daisy_nfm_scores_users, then
        ops.rank_rows_f32; the eval kernel computes a pair's score from the pair alone, so the result does not depend
        on chunk_bytes, bit for bit.  Nothing of the model changes: not the running statistics, not the score-call count."""
        U, I, make_scorer = self._full_rank_scorer("full_rank_users")
        return self._full_rank_users_scored(users, exclude, return_scores, chunk_bytes, U, I, self.device, make_scorer,
                                            validate=validate)         # (validate: as in ops.full_rank_users)

    def full_rank_positions(self, users, targets, exclude=None, chunk_bytes=None, **kw):
        """The exact rank of every held-out item among all eligible items (no counterpart in the reference; DESIGN.md
        §28): `targets` and `exclude` are an (indptr, items) device CSR or a dict of sets (test_ur / train_ur); ->
        ops.full_rank_positions' tuple, consistent with full_rank_users - its ids[b, pos] is the target wherever pos <
        topk - without the cap on topk.  Eval mode only, and full_rank_users' chunks: per chunk one
        daisy_nfm_scores_users call and one ops.rank_rows_positions_f32; the result does not depend on chunk_bytes, bit
        for bit.  kw: return_scores, return_eligible, validate."""
        U, I, make_scorer = self._full_rank_scorer("full_rank_positions")
        return self._full_rank_positions_scored(users, targets, exclude, chunk_bytes, U, I, self.device, make_scorer, **kw)

    def _full_rank_scorer(self, what):
        """(user count, item count, make_scorer) of full_rank_users and full_rank_positions: the eval scores of a chunk of
        users against all items through daisy_nfm_scores_users"""
        if self.training:
            raise RuntimeError(f"NFM.{what} ranks in eval mode only (running statistics, no dropout): call "
                               "model.eval() first")
        p = self._params()
        bn = self._bn()
        ctx = self._score_ctx(1)
        U, I = self.embed_user.num_embeddings, self.embed_item.num_embeddings

        def make_scorer(us_all, rows):
            return lambda us, b0, b1, out: ctx.scores_users(p, bn, us, out)

        return U, I, make_scorer
