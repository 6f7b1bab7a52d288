"""NGCF recommender with the reference's interface, trained by HIP kernels.

Mirror of daisy/model/NGCFRecommender.py:62-252 (class ``NGCF``): same config keys, the same ``nn`` modules built in
the same order (so a seed gives the reference's initial parameters and ``state_dict`` keys), same attributes and
methods.  One training step (``calc_loss`` + backward + optimiser step of the reference) is
    out = [E0 | E1 | ... | EL],  E_k = layer_k(A_hat_drop, E_{k-1})     daisy_lgcn_spmm_ex + daisy_ngcf_layer_forward
    loss, coefficients on rows of `out`                                  daisy_bpr_forward / _finalize   (the MF kernels)
    G   = d loss / d out                                                 daisy_bpr_item_grad_data + daisy_bpr_user_grad
    layers L..1: dE_{k-1}, dX, dW, db                                    daisy_ngcf_layer_backward + daisy_ngcf_wgrad_reduce
                 dE_{k-1} += A_hat_drop^T dX                             daisy_lgcn_spmm_ex (transpose)
    regulariser rows of E0                                               daisy_lgcn_reg_grad
    Adam / SGD on one flat buffer holding every parameter                daisy_adam_dense / daisy_sgd_dense
Like the reference, the propagation is recomputed for every batch.  There is no CPU path.

Dropout streams differ from the reference (device counter hash instead of torch.rand; DESIGN.md "NGCF"), and, like
the reference, message dropout also acts in eval mode: ``nn.Dropout`` is built inside ``forward`` and a fresh module
is in training mode, so ``rank`` / ``full_rank`` / ``predict`` see it too.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .. import _native as N
from ._flat import flatten_parameters, views_live, views_of
from .AbstractRecommender import GeneralRecommender


class BiGNN(nn.Module):
    """NGCFRecommender.py:38-60: the parameters of one layer (the computation is daisy_ngcf_layer_forward)."""

    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.in_dim = in_dim
        self.out_dim = out_dim
        self.linear = torch.nn.Linear(in_features=in_dim, out_features=out_dim)
        self.interact_transform = torch.nn.Linear(in_features=in_dim, out_features=out_dim)


class NGCF(GeneralRecommender):
    def __init__(self, config):
        """Config keys as in NGCFRecommender.py:63-122."""
        super().__init__(config)
        self.epochs = config["epochs"]
        self.lr = config["lr"]
        self.topk = config["topk"]
        self.user_num = config["user_num"]
        self.item_num = config["item_num"]
        self.interaction_matrix = config["inter_matrix"]
        self.embedding_size = config["factors"]
        hidden = config.get("hidden_size_list")
        self.hidden_size_list = [self.embedding_size] + list(hidden if hidden is not None else [64, 64, 64])
        widths = [int(w) for w in self.hidden_size_list]
        if any(w < 1 or w > N.NGCF_MAX_WIDTH for w in widths) or sum(widths) > 512:
            raise ValueError(f"NGCF: widths {widths} unsupported (each 1..{N.NGCF_MAX_WIDTH}, concatenated <= 512)")
        self.node_dropout = float(config["node_dropout"])
        self.message_dropout = float(config["mess_dropout"])
        self.reg_1 = config["reg_1"]
        self.reg_2 = config["reg_2"]

        self.embed_user = nn.Embedding(self.user_num, self.embedding_size)
        self.embed_item = nn.Embedding(self.item_num, self.embedding_size)
        self.gnn_layers = torch.nn.ModuleList()
        for in_size, out_size in zip(self.hidden_size_list[:-1], self.hidden_size_list[1:]):
            self.gnn_layers.append(BiGNN(in_size, out_size))

        self.restore_user_e = None
        self.restore_item_e = None

        self.loss_type = config["loss_type"]
        self.optimizer = config["optimizer"] if config["optimizer"] != "default" else "adam"
        self.initializer = config["init_method"] if config["init_method"] != "default" else "xavier_normal"
        self.early_stop = config["early_stop"]
        self.apply(self._init_weight)

        # knob of the native path, as in LightGCN: 'sorted' = bitwise reproducible run to run (the item gradient is
        # owner-summed; the graph products and the layer kernels are always reproducible), 'chunked' = throughput
        self.item_mode = str(config.get("item_mode", "chunked")).lower()
        # dropout keys: (seed, forward call) -> counter hash on the device
        self._seed = int(config.get("seed", 0)) & 0xFFFFFFFF
        self._calls = 0
        self._flat = None
        self._graph = None
        self._bufs = None

    # -- device state ------------------------------------------------------------------------------
    @property
    def _widths(self):
        return [int(w) for w in self.hidden_size_list]

    def _params(self):
        """Every parameter as a view of ONE flat device buffer (named_parameters order)."""
        self._require_device()
        if not views_live(self._flat, self.parameters()):
            self._flat = flatten_parameters(self.named_parameters(), self.device)
            self._gflat = torch.zeros_like(self._flat)
            self._grads = views_of(self._gflat, self.named_parameters())
        return self._flat

    def _ego(self):
        """the [P; Q] rows of the flat buffer `_params` has homed (a step reads them several times: no liveness walk here)"""
        U, I, d = self.user_num, self.item_num, self.embedding_size
        return self._flat[:(U + I) * d].view(U + I, d)

    def _adj(self):
        """get_norm_adj_mat (:124-144) on the device, built once (the LightGCN graph)."""
        if self._graph is None:
            m = self.interaction_matrix.tocoo()
            if isinstance(m.row, torch.Tensor):     # utils.get_inter_matrix's device columns: no scipy, no second upload
                users, items = m.row.to(self.device), m.col.to(self.device)
            else:
                users = torch.as_tensor(np.ascontiguousarray(m.row)).to(self.device)
                items = torch.as_tensor(np.ascontiguousarray(m.col)).to(self.device)
            self._graph = ops.LgcnGraph(users, items, self.user_num, self.item_num)
            self._graph.set_reproducible(self.item_mode == "sorted")
        return self._graph

    def _work(self):
        """Per-model buffers: the concat table, its gradient, per-layer X and norms, the backward scratch."""
        if self._bufs is None:
            w, n = self._widths, self.user_num + self.item_num
            D, dev = sum(w), self.device
            f32 = dict(dtype=torch.float32, device=dev)
            ws = max(ops.ngcf_ws_bytes(n, a, b) for a, b in zip(w[:-1], w[1:])) if len(w) > 1 else 256
            self._bufs = dict(out=torch.empty(n, D, **f32), G=torch.empty(n, D, **f32),
                              X=[torch.empty(n, a, **f32) for a in w[:-1]], norm=[torch.empty(n, **f32) for _ in w[1:]],
                              dE=[torch.empty(n * max(w), **f32) for _ in range(2)], dX=torch.empty(n * max(w), **f32),
                              ws=torch.empty(max(ws, 256), dtype=torch.uint8, device=dev))
        return self._bufs

    def _offsets(self):
        w = self._widths
        return [sum(w[:k]) for k in range(len(w))]

    def _propagate(self, out, node, X=None, norm=None):
        """forward (:158-172) into the concat buffer `out` [N, D]; node: apply node dropout (training mode).
        Returns the dropout seed of this call."""
        self._calls += 1
        seed = (self._seed << 32) | (self._calls & 0xFFFFFFFF)
        w, off = self._widths, self._offsets()
        b = self._work()
        E0 = self._ego()
        out[:, :w[0]].copy_(E0)
        g = self._adj()
        keep = (self.node_dropout, seed) if (node and self.node_dropout != 0) else None
        for k, gnn in enumerate(self.gnn_layers):
            E = out[:, off[k]:off[k] + w[k]]
            Xk = X[k] if X is not None else b["X"][k]
            nk = norm[k] if norm is not None else b["norm"][k]
            g.spmm_ex(E, out=Xk, keep=keep)
            ops.ngcf_layer_forward(E, Xk, gnn.linear.weight, gnn.linear.bias, gnn.interact_transform.weight,
                                   gnn.interact_transform.bias, out[:, off[k + 1]:off[k + 1] + w[k + 1]], nk,
                                   self.message_dropout, seed, k)
        return seed

    def forward(self):
        """:158-172 -> (user_all_embeddings [U, D], item_all_embeddings [I, D])"""
        self._params()
        b = self._work()
        out = torch.empty_like(b["out"])
        X = [torch.empty_like(x) for x in b["X"]]
        norm = [torch.empty_like(x) for x in b["norm"]]
        self._propagate(out, self.training, X, norm)
        return out[:self.user_num], out[self.user_num:]

    def _backward(self, G, seed, node):
        """d loss / d parameters from G = d loss / d out: into the flat gradient buffer (E0 rows written, the layer
        weights accumulated)."""
        w, off = self._widths, self._offsets()
        b = self._work()
        n = self.user_num + self.item_num
        g = self._adj()
        keep = (self.node_dropout, seed) if (node and self.node_dropout != 0) else None
        out = b["out"]
        dE0 = self._gflat[:n * w[0]].view(n, w[0])
        L = len(self.gnn_layers)
        dY = G[:, off[L]:off[L] + w[L]]
        for k in range(L - 1, -1, -1):
            gnn = self.gnn_layers[k]
            dE = dE0 if k == 0 else b["dE"][k & 1][:n * w[k]].view(n, w[k])
            dX = b["dX"][:n * w[k]].view(n, w[k])
            ops.ngcf_layer_backward(dY, out[:, off[k + 1]:off[k + 1] + w[k + 1]], b["norm"][k],
                                    out[:, off[k]:off[k] + w[k]], b["X"][k], gnn.linear.weight,
                                    gnn.interact_transform.weight, dE, dX, b["ws"], self.message_dropout, seed, k,
                                    gprev=G[:, off[k]:off[k] + w[k]])
            p = f"gnn_layers.{k}."
            ops.ngcf_wgrad_reduce(b["ws"], n, w[k], w[k + 1], self._grads[p + "linear.weight"],
                                  self._grads[p + "linear.bias"], self._grads[p + "interact_transform.weight"],
                                  self._grads[p + "interact_transform.bias"])
            g.spmm_ex(dX, out=dE, accumulate=True, keep=keep, transpose=True)
            dY = dE

    def _batch_grads(self, ctx, ctx_ego, u, i, j, loss_id):
        """loss (left in ctx.stats) and d loss / d parameters accumulated into the flat gradient buffer."""
        U = self.user_num
        reg = self.reg_1 != 0 or self.reg_2 != 0
        pointwise = loss_id in ops.POINTWISE_LOSSES
        b = self._work()
        out, G = b["out"], b["G"]
        seed = self._propagate(out, True)
        ctx.set_batch(u, i, j)
        if reg:                       # the regularisers act on the EGO rows (:186-205): their sums first
            E0 = self._ego()
            ctx_ego.set_batch(u, i, j)
            ctx_ego.forward(E0[:U], E0[U:], loss_id)
        ctx.forward(out[:U], out[U:], loss_id)
        if reg:
            ctx.stats[1:7] = ctx_ego.stats[1:7]
        else:
            ctx.stats[1:7] = 0
        ctx.finalize(self.reg_1, self.reg_2, accumulate=True)
        G.zero_()
        if self.item_mode == "sorted":
            ctx.item_grad(out[:U], out[U:], 0.0, 0.0, N.ITEM_SORTED, gQ=G[U:])
        else:
            ctx.item_grad_data(out[:U], out[U:], N.ITEM_CHUNKED, gQ=G[U:])
        ctx.user_grad(out[:U], out[U:], 0.0, 0.0, G[:U])
        self._backward(G, seed, True)
        if reg:
            ops.lgcn_reg_grad(self._ego(), u, i, j, U, pointwise, self.reg_1, self.reg_2, ctx.stats,
                              self._gflat[:(U + self.item_num) * self.embedding_size].view(-1, self.embedding_size))

    def _contexts(self, B, loss_id):
        ctx = ops.BprContext(B, sum(self._widths), self.user_num, self.item_num, device=self.device)
        ctx_ego = ops.BprContext(B, self.embedding_size, self.user_num, self.item_num, device=self.device)
        for c in (ctx, ctx_ego):
            c.set_pointwise(loss_id in ops.POINTWISE_LOSSES)
        return ctx, ctx_ego

    def calc_loss(self, batch):
        """:174-209: the batch loss (0-dim float64 device tensor; no autograd graph, no parameter change)."""
        loss_id = self._build_criterion(self.loss_type)
        self.restore_user_e, self.restore_item_e = None, None
        self._params()
        u, i, j = (torch.as_tensor(x).to(torch.int32).to(self.device).contiguous() for x in batch[:3])
        ctx, ctx_ego = self._contexts(u.numel(), loss_id)
        saved = self._gflat.clone()
        try:
            self._batch_grads(ctx, ctx_ego, u, i, j, loss_id)
            return ctx.stats[N.ST_LOSS].clone()
        finally:
            self._gflat.copy_(saved)
            ctx.close()
            ctx_ego.close()

    def fit(self, train_loader):
        """AbstractRecommender.py:103-137 for NGCF (one full propagation per batch, as the reference)."""
        opt = self._resolve_optimizer()
        loss_id = self._build_criterion(self.loss_type)
        flat = self._params()
        self.restore_user_e, self.restore_item_e = None, None
        triples, n, B = self._train_rows(train_loader)
        optim = ops.DenseOptimizer(opt, self.lr)
        ctx, ctx_ego = self._contexts(min(B, max(n, 1)), loss_id)

        def run_epoch(epoch):
            ctx.epoch_acc.zero_()
            if n > 0:
                order = self._epoch_rows(train_loader, triples, n)
                for s in range(0, n, B):
                    rows = order[s:s + B]
                    u, i, j = (rows[:, k].contiguous() for k in range(3))
                    self._batch_grads(ctx, ctx_ego, u, i, j, loss_id)
                    optim.next_step()
                    optim.step(flat, self._gflat)          # also clears the gradient
            acc = ctx.epoch_acc.cpu()
            return float(acc[0]), float(acc[1])

        try:
            self._run_epochs(run_epoch)
        finally:
            torch.cuda.synchronize()
            ctx.close()
            ctx_ego.close()

    def _restore(self):
        if self.restore_user_e is None or self.restore_item_e is None:
            self.restore_user_e, self.restore_item_e = self.forward()
        return self.restore_user_e, self.restore_item_e

    def predict(self, u, i):
        """:211-219"""
        ue, ie = self._restore()
        return float(ops.mf_predict(ue, ie, torch.tensor([u], device=self.device),
                                    torch.tensor([i], device=self.device)).cpu().item())

    def rank(self, test_loader):
        """:221-240 -> float32 [n_users, topk] like the reference."""
        ue, ie = self._restore()
        return self._rank_loader(test_loader, lambda us, cands_ids: ops.mf_rank_topk(ue, ie, us, cands_ids, self.topk))

    def full_rank(self, u):
        """:242-252 -> int64 [topk]"""
        ue, ie = self._restore()
        return ops.mf_full_rank(ue, ie, int(u), self.topk).cpu().numpy()

    def full_rank_positions(self, users, targets, exclude=None, **kw):
        """exact ranks of held-out items over the propagated embeddings (MF.full_rank_positions)"""
        ue, ie = self._restore()
        return self._full_rank_positions(ue, ie, users, targets, exclude, **kw)

    def full_rank_users(self, users, exclude=None, return_scores=False):
        """full ranking of many users over the propagated embeddings (MF.full_rank_users)"""
        ue, ie = self._restore()
        return self._full_rank_users(ue, ie, users, exclude, return_scores)
