"""Multi-VAE (VAECF) recommender with the reference's interface, trained by HIP kernels.

Mirror of daisy/model/VAECFRecommender.py (class ``VAECF``, an ``AERecommender``): same config keys, attributes
(``update``, ``history_item_id``, ``encode_layer_dims``, ...) and methods, and the ``nn`` modules built in the same order,
so a seed gives the reference's initial parameters and ``state_dict`` keys and shapes.  ``fit`` / ``calc_loss`` /
``rank`` / ``full_rank`` / ``predict`` run through ``daisy_vae_*`` (include/daisyrec_amd.h, csrc/vae.hip): the sparse
first encoder layer over the users' history rows, every dense layer, the reparameterisation, the log-softmax
cross-entropy + annealed KL and the backward pass, then one dense optimiser pass over the flat parameter buffer.
There is no CPU path.

``encoder.0.weight`` ([hidden0, item_num] in torch) is held item-major behind a transposed view: ``state_dict()``,
``load_state_dict()`` and ``parameters()`` show the reference's shape.  Dropout and the reparameterisation noise use
the device's counter hash, not torch's generator: the same distributions, a different stream.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from .. import _native as N
from ._flat import flatten_parameters, views_live
from .AbstractRecommender import AERecommender


class VAECF(AERecommender):
    def __init__(self, config):
        """Config keys as in VAECFRecommender.py:18-61 (multi-vae.yaml + basic.yaml)."""
        super().__init__(config)
        self.epochs = config["epochs"]
        self.lr = config["lr"]
        self.dropout = config["dropout"]

        self.layers = config["mlp_hidden_size"] if config["mlp_hidden_size"] is not None else [600]
        self.lat_dim = config["latent_dim"]
        self.anneal_cap = config["anneal_cap"]
        self.total_anneal_steps = config["total_anneal_steps"]

        self.user_num = config["user_num"]
        self.item_num = config["item_num"]

        # config['history_csr'] (utils.history_csr: the users' rows as a device CSR, built from the interactions alone):
        # the padded pair is then optional
        self.history_csr = config.get("history_csr")
        hid = config.get("history_item_id") if self.history_csr is not None else config["history_item_id"]
        hval = config.get("history_item_value") if self.history_csr is not None else config["history_item_value"]
        self.history_item_id = None if hid is None else hid.to(self.device)
        self.history_item_value = None if hval is None else hval.to(self.device)
        self.update = 0

        self.encode_layer_dims = [self.item_num] + self.layers + [self.lat_dim]
        self.decode_layer_dims = [int(self.lat_dim / 2)] + self.encode_layer_dims[::-1][1:]
        if len(self.layers) > N.VAE_MAX_HIDDEN or int(self.lat_dim) < 2:
            raise ValueError(f"VAECF: mlp_hidden_size={self.layers} (at most {N.VAE_MAX_HIDDEN} layers), "
                             f"latent_dim={self.lat_dim} (>= 2) unsupported")

        self.encoder = self.mlp_layers(self.encode_layer_dims)
        self.decoder = self.mlp_layers(self.decode_layer_dims)

        self.optimizer = config["optimizer"] if config["optimizer"] != "default" else "adam"
        self.initializer = config["init_method"] if config["init_method"] != "default" else "xavier_normal"
        self.early_stop = config["early_stop"]

        self.apply(self._init_weight)
        self.topk = config["topk"]

        self._flat = None
        self._csr_cache = None
        self._sctx = None
        self._steps = 0           # optimiser steps taken: the noise key of step k is (seed << 32) | k
        self._score_calls = 0

    def mlp_layers(self, layer_dims):
        """VAECFRecommender.py:63-69: Linear layers, Tanh between them."""
        mods = []
        for k, (d_in, d_out) in enumerate(zip(layer_dims[:-1], layer_dims[1:])):
            mods.append(nn.Linear(d_in, d_out))
            if k != len(layer_dims) - 2:
                mods.append(nn.Tanh())
        return nn.Sequential(*mods)

    # -- parameters as the kernels see them: ONE flat device buffer, the module's tensors are views -------------------
    def _params(self):
        """Move the parameters into one contiguous device buffer (once; encoder.0.weight item-major), return it."""
        self._require_device()
        if not views_live(self._flat, self.parameters()):
            self._flat = flatten_parameters(self.named_parameters(), self.device, transposed=("encoder.0.weight",))
        return self._flat

    def _csr(self):
        """The user rows of R on the device (ops.vae_history_csr), rebuilt when the history tensors change; also the
        rows' entry counts on the host (the per-batch entry counts the kernels are given)."""
        if self.history_csr is not None:
            key = ("csr", id(self.history_csr))
            if self._csr_cache is None or self._csr_cache[0] != key:
                csr = self._checked_csr(self.history_csr)
                self._csr_cache = (key, csr, (csr[0][1:] - csr[0][:-1]).cpu())
            return self._csr_cache[1], self._csr_cache[2]
        key = (id(self.history_item_id), id(self.history_item_value))
        if self._csr_cache is None or self._csr_cache[0] != key:
            hid = self.history_item_id.to(self.device)
            hval = self.history_item_value.to(self.device)
            csr = ops.vae_history_csr(hid, hval, self.item_num)
            lens = (csr[0][1:] - csr[0][:-1]).cpu()
            self._csr_cache = (key, csr, lens)
        return self._csr_cache[1], self._csr_cache[2]

    def _checked_csr(self, given):
        """config['history_csr'] = (row_ptr int64 [user_num + 1], col int32 [nnz], val float32 [nnz][, L]) as
        utils.history_csr returns it: shapes, dtypes, row_ptr and the column range are checked before a kernel reads it."""
        if not isinstance(given, (tuple, list)) or len(given) not in (3, 4):
            raise TypeError("config['history_csr']: expected (row_ptr, col, val) or (row_ptr, col, val, L)")
        row_ptr, col, val = (torch.as_tensor(t).to(self.device).contiguous() for t in given[:3])
        if row_ptr.dtype != torch.int64 or col.dtype != torch.int32 or val.dtype != torch.float32:
            raise TypeError(f"config['history_csr']: expected int64 / int32 / float32 tensors, got {row_ptr.dtype}, {col.dtype}, "
                            f"{val.dtype}")
        if row_ptr.dim() != 1 or row_ptr.numel() != int(self.user_num) + 1 or col.dim() != 1 or val.shape != col.shape:
            raise ValueError(f"config['history_csr']: expected row_ptr [{int(self.user_num) + 1}] and col / val [nnz], got "
                             f"{tuple(row_ptr.shape)}, {tuple(col.shape)}, {tuple(val.shape)}")
        if int(row_ptr[0]) != 0 or int(row_ptr[-1]) != col.numel() or bool((row_ptr[1:] < row_ptr[:-1]).any()):
            raise ValueError(f"config['history_csr']: row_ptr must ascend from 0 to nnz = {col.numel()}")
        if col.numel() and (int(col.min()) < 0 or int(col.max()) >= int(self.item_num)):
            raise IndexError(f"index out of range: history item ids must lie in [0, {int(self.item_num)})")
        return row_ptr, col, val

    def get_user_rating_matrix(self, user):
        """AbstractRecommender.py:147-158 -> [B, item_num]; with config['history_csr'] the asked rows are densified from
        the CSR (the same rows: the CSR is what index_put_ leaves of the padded pair)."""
        if self.history_csr is None:
            return super().get_user_rating_matrix(user)
        (row_ptr, col, val), _ = self._csr()
        rows = torch.as_tensor(user).to(self.device).long().reshape(-1)
        self._check_users(rows)
        out = torch.zeros(rows.numel(), self.item_num, dtype=torch.float32, device=self.device)
        lens = row_ptr[rows + 1] - row_ptr[rows]
        total = int(lens.sum()) if rows.numel() else 0
        if total:
            which = torch.repeat_interleave(torch.arange(rows.numel(), device=self.device), lens)
            begin = torch.cumsum(lens, 0) - lens
            src = row_ptr[rows][which] + (torch.arange(total, device=self.device) - begin[which])
            out[which, col[src].long()] = val[src]
        return out

    def _check_users(self, users):
        U = int(self.user_num) if self.history_csr is not None else int(self.history_item_id.shape[0])
        if users.numel() and (int(users.min()) < 0 or int(users.max()) >= U):
            raise IndexError(f"index {int(users.max()) if int(users.max()) >= U else int(users.min())} is out of bounds "
                             f"for dimension 0 with size {U}")

    def _check_items(self, items):
        if items.numel() and (int(items.min()) < 0 or int(items.max()) >= self.item_num):
            raise IndexError(f"index out of range: item ids must lie in [0, {self.item_num})")

    def _ctx(self, rows, entries):
        return ops.VaeContext(max(int(rows), 1), max(int(entries), 1), self.item_num, self.layers, self.lat_dim,
                              device=self.device)

    def _score_ctx(self, rows, entries):
        ctx = self._sctx
        if ctx is None or ctx.max_batch < rows or ctx.max_entries < entries:
            if ctx is not None:
                ctx.close()
            ctx = self._sctx = self._ctx(max(rows, 1 if ctx is None else ctx.max_batch),
                                         max(entries, 1 if ctx is None else ctx.max_entries))
        return ctx

    def _scores(self, users, items=None, keep=None, eps=None):
        """VAECF.forward's scores in the module's mode: [B, C] for candidates items [B, C], or [B, item_num]."""
        W = self._params()
        csr, lens = self._csr()
        users = torch.as_tensor(users).reshape(-1).to(torch.int64)
        self._check_users(users)
        entries = int(lens[users.cpu()].sum()) if users.numel() else 0
        ctx = self._score_ctx(users.numel(), entries)
        train = bool(self.training)
        self._score_calls += 1
        return ctx.scores(W, csr, users.to(self.device), entries, items=items, train=train,
                          dropout=self.dropout if train else 0.0, seed=self._seed_hi | (0x80000000 + self._score_calls),
                          keep=keep, eps=eps)

    # -- reference surface -------------------------------------------------------------------------------------------
    def reparameterize(self, mu, logvar):
        """VAECFRecommender.py:71-77 (torch's generator; the kernels draw eps from the device hash)."""
        if self.training:
            std = torch.exp(0.5 * logvar)
            return torch.randn_like(std).mul(std).add_(mu)
        return mu

    def forward(self, rating_matrix):
        """VAECFRecommender.py:79-90 needs the encoder output of a dense rating matrix; the HIP path scores users from
        their history rows instead (rank / full_rank / predict)."""
        raise NotImplementedError("VAECF.forward(rating_matrix): the HIP path scores users from their history rows "
                                  "(rank / full_rank / predict); there is no dense-input path")

    def calc_loss(self, batch):
        """VAECFRecommender.py:92-110: the batch loss (0-dim float64 device tensor, no autograd graph, no parameter
        change); counts `update` like the reference.  Training-mode noise uses the key of the next optimiser step."""
        W = self._params()
        csr, lens = self._csr()
        user = torch.as_tensor(batch).reshape(-1).to(torch.int64)
        self._check_users(user)
        self.update += 1
        if self.total_anneal_steps > 0:
            anneal = min(self.anneal_cap, 1. * self.update / self.total_anneal_steps)
        else:
            anneal = self.anneal_cap
        entries = int(lens[user.cpu()].sum())
        ctx = self._ctx(user.numel(), entries)
        try:
            g = torch.zeros_like(W)
            ctx.step_grads(W, g, csr, user.to(self.device), entries, train=self.training,
                           dropout=self.dropout if self.training else 0.0, anneal=anneal,
                           seed=self._seed_hi | (self._steps + 1))
            return ctx.stats[N.VST_LOSS].clone()
        finally:
            ctx.close()

    def fit(self, train_loader):
        """AbstractRecommender.py:103-137 for VAECF: the epoch's steps (daisy_vae_step_grads + the dense optimiser) are
        issued by the library in one call; one host sync per epoch (the NaN check is per epoch)."""
        self._require_device()
        opt = self._resolve_optimizer()
        W = self._params()
        csr, lens = self._csr()
        users_all, n, B = self._train_rows(train_loader, columns=1, expects="AEDataset (dataset.data = the training users)")
        self._check_users(users_all[:n])
        ulens = lens[users_all]
        max_entries = int(torch.topk(ulens, min(B, ulens.numel())).values.sum()) if ulens.numel() else 0
        g = torch.zeros_like(W)
        optim = ops.DenseOptimizer(opt, self.lr)         # a fresh optimiser per fit, as the reference builds one
        ctx = self._ctx(min(B, max(n, 1)), max_entries)

        def run_epoch(epoch):
            order = self._epoch_rows(train_loader, users_all, n)      # (drop_last: the order's first n positions)
            ctx.stats.zero_()
            if n > 0:
                entries = [int(x.sum()) for x in torch.split(lens[order], B)]
                steps = ctx.fit_epoch(W, g, csr, order.to(self.device), B, entries, optim, self.dropout,
                                      self.anneal_cap, self.total_anneal_steps, self.update,
                                      seed_hi=self._seed_hi, step0=self._steps)
                self._steps += steps
                self.update += steps
            st = ctx.stats.cpu()
            return float(st[N.VST_LOSS_SUM]), float(st[N.VST_NONFINITE])

        try:
            self._run_epochs(run_epoch)
        finally:
            torch.cuda.synchronize()
            ctx.close()

    def predict(self, u, i):
        """VAECFRecommender.py:112-119 -> one float."""
        items = torch.tensor([[int(i)]], dtype=torch.int64)
        self._check_items(items)
        return float(self._scores(torch.tensor([int(u)]), items.to(self.device)).cpu().item())

    def rank(self, test_loader):
        """VAECFRecommender.py:121-138 -> float32 [n_users, topk] like the reference; only the candidates' rows of the
        last layer are evaluated."""
        self._params()

        def topk_of(us, cands_ids):
            cands_ids = cands_ids.to(torch.int64)
            self._check_items(cands_ids)
            return ops.topk_from_scores(self._scores(us, cands_ids), cands_ids, self.topk)

        return self._rank_loader(test_loader, topk_of)

    def full_rank(self, u):
        """VAECFRecommender.py:140-145 -> int64 [topk] over all items (training items included)."""
        scores = self._scores(torch.tensor([int(u)]))
        return ops.full_topk_from_scores(scores.view(-1), self.topk).cpu().numpy()

    def full_rank_users(self, users, exclude=None, return_scores=False, chunk_bytes=None, validate=True):
        """Full ranking of many users (no counterpart in the reference): device int64 [len(users),
        min(topk, I)], best first, without the items of the user's row of `exclude` (None, an (indptr, items) device CSR
        or a train_ur dict of sets) - the protocol Multi-VAE is evaluated under; -1 where a user has fewer eligible items
        than topk.  return_scores: (ids, float32 scores).  Eval mode only - dropout and the reparameterisation noise over
        an arbitrary chunk are not a ranking: call model.eval() first.  chunk_bytes (default 256 MiB) of scores at a time
        through daisy_vae_scores in the shared score context (config['history_csr'] works as for rank), then
        ops.rank_rows_f32.  The GEMMs pick their split-K from the call's row count and the context's workspace, so the bits
        of a score depend on the chunk: the promise is per chunk - the chunk's lists are the exact ranking of what
        `_scores` returns for exactly that chunk's users in the same context.  Neither `update` nor the score-call count
        changes."""
        U, make_scorer = self._full_rank_scorer("full_rank_users")
        return self._full_rank_users_scored(users, exclude, return_scores, chunk_bytes, U, self.item_num, self.device,
                                            make_scorer, validate=validate)

    def full_rank_positions(self, users, targets, exclude=None, chunk_bytes=None, **kw):
        """The exact rank of every held-out item among all eligible items (no counterpart in the reference; DESIGN.md
        §28) - the full-ranking protocol Multi-VAE is defined under, without a cap on the cutoff: `targets` and `exclude`
        are an (indptr, items) device CSR or a dict of sets (test_ur / train_ur); -> ops.full_rank_positions' tuple.  Eval
        mode only, and full_rank_users' chunks: per chunk one daisy_vae_scores call and one ops.rank_rows_positions_f32, so
        with the same chunk_bytes full_rank_users' ids[b, pos] is the target wherever pos < topk (a score's bits are per
        chunk, as there).  kw: return_scores, return_eligible, validate."""
        U, make_scorer = self._full_rank_scorer("full_rank_positions")
        return self._full_rank_positions_scored(users, targets, exclude, chunk_bytes, U, self.item_num, self.device,
                                                make_scorer, **kw)

    def _full_rank_scorer(self, what):
        """(user count, make_scorer) of full_rank_users and full_rank_positions: the scores of a chunk of users against all
        items through daisy_vae_scores in the shared score context"""
        if self.training:
            raise RuntimeError(f"VAECF.{what} ranks in eval mode only (no dropout, no reparameterisation noise): "
                               "call model.eval() first")
        W = self._params()
        csr, lens = self._csr()
        U = int(self.user_num) if self.history_csr is not None else int(self.history_item_id.shape[0])

        def make_scorer(us_all, rows):
            # the chunks' entry counts from the host copy of the row lengths: one copy of the ids, nothing per chunk
            ulens = lens[us_all.cpu()]
            entries = [int(x.sum()) for x in torch.split(ulens, rows)]
            ctx = self._score_ctx(rows, max(entries))
            return lambda us, b0, b1, out: ctx.scores(W, csr, us, entries[b0 // rows], out=out)

        return U, make_scorer

