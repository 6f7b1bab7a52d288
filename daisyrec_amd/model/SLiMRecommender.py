"""SLiM (sparse linear method) with the reference's interface, fitted by HIP kernels.

Mirror of daisy/model/SLiMRecommender.py (class ``SLiM``): same config keys (``alpha``, ``elastic``, ``topk``,
``user_num``, ``item_num``), ``fit(train_set)`` takes the training DataFrame, ``predict`` / ``rank`` / ``full_rank``
return the reference's types.  The reference fits one scikit-learn ``ElasticNet(positive=True, precompute=True)`` per
item column; here the Gram matrix ``G = X^T X`` is formed once on the fp32 MFMA product (``daisy_slim_gram``), every
column's coordinate descent runs over it in fp64 (``daisy_slim_cd``, one workgroup per column) and the scores
``A_tilde[u, i] = X[u, :] . W[:, i]`` are computed per request from the truncated ``W`` (``daisy_slim_scores``).  There is
no CPU path.

Deviations: the coordinates are visited in cyclic order instead of scikit-learn's random order (for
``elastic < 1`` both converge to the same unique minimiser; the result is deterministic); ties are ranked in stable
order; ``A_tilde`` is not stored: the property builds the dense matrix on demand and is meant for small problems only.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .. import _native as N
from ._frame import FrameRecommender

_SLAB_BYTES = 256 << 20        # default config['slim_slab_bytes']


class SLiM(FrameRecommender):
    _name = "SLiM"
    _users_op = staticmethod(ops.slim_full_rank_users)
    _positions_op = staticmethod(ops.slim_full_rank_positions)

    def __init__(self, config):
        """Config keys as in SLiMRecommender.py:28-57 (slim.yaml + basic.yaml); ``slim_tol`` (1e-4) and
        ``slim_max_iter`` (100) are the two values the reference hard-codes in its ElasticNet; ``slim_slab_bytes`` (256 MB)
        bounds the (row, value) output slab of one daisy_slim_cd call: a fit whose slab would be larger runs column chunk
        by column chunk (same result)."""
        super().__init__(config)
        self.alpha = float(config["alpha"])
        self.elastic = float(config["elastic"])
        self.tol = float(config.get("slim_tol", 1e-4))
        self.max_iter = int(config.get("slim_max_iter", 100))
        self.slab_bytes = int(config.get("slim_slab_bytes", _SLAB_BYTES))
        self.item_num = int(config["item_num"])
        self.user_num = int(config["user_num"])
        self.topk = int(config["topk"])
        if not self.alpha > 0:
            raise ValueError(f"SLiM: alpha={self.alpha} must be positive")
        if not 0.0 <= self.elastic <= 1.0:
            raise ValueError(f"SLiM: elastic={self.elastic} must lie in [0, 1]")
        if not 1 <= self.topk <= N.SLIM_MAX_TOPK:
            raise ValueError(f"SLiM: topk={self.topk} must lie in [1, {N.SLIM_MAX_TOPK}]")
        if self.user_num < 1 or self.item_num < 1:
            raise ValueError(f"SLiM: user_num={self.user_num}, item_num={self.item_num} must be positive")
        if self.max_iter < 1 or not self.tol >= 0:
            raise ValueError(f"SLiM: slim_max_iter={self.max_iter} (>= 1), slim_tol={self.tol} (>= 0)")
        self._csr = None            # X on the device
        self._W = None              # the truncated W by column on the device
        self.fit_info = None
        self.logger.info(f"user num: {self.user_num}, item num: {self.item_num}")

    # -- fit -----------------------------------------------------------------------------------------------------------
    def fit(self, train_set, verbose=True):
        """SLiMRecommender.py:59-124: Gram matrix, the columns' elastic nets, truncation; W and X stay on the device.
        The frame's columns are 'user', 'item', 'rating' (SLiMRecommender.py:148-157 hard-codes them)."""
        csr, _ = self._frame_csr(train_set)
        I, k = self.item_num, self.topk
        G = ops.slim_gram(csr, I)
        chunk = max(1, min(I, self.slab_bytes // (8 * k)))
        parts = []
        for col0 in range(0, I, chunk):
            parts.append(ops.slim_fit(G, self.user_num, self.alpha, self.elastic, k, tol=self.tol, max_iter=self.max_iter,
                                      col0=col0, ncols=min(chunk, I - col0)))
            if verbose:
                done = min(col0 + chunk, I)
                self.logger.info(f"SLIM-ElasticNet-Recommender: enqueued {done} ( {100.0 * done / I:.2f}% ) columns")
        count, rows, vals, sweeps, gap = (torch.cat(x, 0) for x in zip(*parts))
        self._W = ops.slim_columns(count, rows, vals, I)
        self._csr = csr
        self.fit_info = {"sweeps": sweeps.cpu().numpy(), "gap": gap.cpu().numpy()}
        del G

    def _has_fit(self):
        return self._W is not None

    # -- scores: float32, ranked through ops.topk_from_scores; full_rank_users and full_rank_positions are the base's ------
    def _operands(self):
        return self._csr, self._W, self.item_num

    def _check_users(self, users):
        self._check(users, self.user_num, "user")

    def _check_items(self, items):
        self._check(items, self.item_num, "item")

    def _scores(self, users, items=None):
        users, items = self._request(users, items)
        return ops.slim_scores(self._csr, self._W, self.item_num, users, items)

    def predict(self, u, i):
        """SLiMRecommender.py:126-127 -> one float (A_tilde[u, i])."""
        return float(self._scores([int(u)], torch.tensor([[int(i)]], dtype=torch.int64)).cpu().item())

    def rank(self, test_loader):
        """SLiMRecommender.py:129-141 -> the candidates' ids [n_users, topk], best first."""
        self._fitted()

        def topk_of(us, cands_ids):
            cands_ids = cands_ids.to(torch.int64)
            return ops.topk_from_scores(self._scores(us, cands_ids), cands_ids, min(self.topk, cands_ids.shape[1]))

        return self._rank_loader(test_loader, topk_of).astype(np.int64)      # (the reference returns the int64 ids)

    def full_rank(self, u):
        """SLiMRecommender.py:143-146 -> int64 [topk] over all items."""
        scores = self._scores([int(u)])
        return ops.full_topk_from_scores(scores.view(-1), min(self.topk, self.item_num)).cpu().numpy()

    # -- the reference's attributes, built on demand -------------------------------------------------------------------
    @property
    def w_sparse(self):
        """SLiMRecommender.py:120-121: scipy.sparse.csr_matrix float32 [item_num, item_num], w_sparse[r, j] = coefficient
        of item r in column j; None before fit."""
        if self._W is None:
            return None
        import scipy.sparse as sp
        w_ptr, w_row, w_val = (t.cpu().numpy() for t in self._W)
        w_row, w_val = w_row[:w_ptr[-1]], w_val[:w_ptr[-1]]
        csc = sp.csc_matrix((w_val, w_row, w_ptr), shape=(self.item_num, self.item_num), dtype=np.float32)
        return csc.tocsr()

    @property
    def A_tilde(self):
        """SLiMRecommender.py:123-124 as a dense float64 [user_num, item_num] array, built on every access from the
        device scores (each an fp64 sum rounded to float32): for small problems only; rank / full_rank / predict do not
        use it.  None before fit."""
        if self._W is None:
            return None
        out = np.empty((self.user_num, self.item_num), dtype=np.float64)
        step = max(1, (64 << 20) // (4 * self.item_num))
        for u0 in range(0, self.user_num, step):
            us = torch.arange(u0, min(u0 + step, self.user_num), dtype=torch.int64)
            out[u0:u0 + us.numel()] = self._scores(us).cpu().numpy()
        return out
