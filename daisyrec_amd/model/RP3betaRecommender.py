"""RP3beta and P3alpha: the graph random-walk baselines, fitted by a HIP sparse two-hop walk with a per-row top-K.

No counterpart in the reference: P3alpha (Cooper et al. 2014) ranks the items by the probability of a
three-step walk user -> item -> user -> item on the bipartite interaction graph, with the transition probabilities raised
to ``alpha``; RP3beta (Paudel et al. 2016) divides the weight of a target item by its popularity raised to ``beta``.
With X the training matrix [user_num, item_num] (binarised when ``implicit``):

    Pui[u, j] = (x_uj / sum_j x_uj)^alpha       Piu[i, u] = (x_ui / sum_u x_ui)^alpha       col_scale[j] = deg(j)^-beta
    W = the ``min(maxk, item_num)`` largest entries of every row of (Piu Pui) diag(col_scale), without the diagonal

and the scores are ``X W``.  ``ops.walk2_topk`` computes W from the two sparse operands without ever forming the dense
[item_num, item_num] product (the work is the number of two-hop paths, the memory item_num * maxk); everything around it
is torch plumbing done once per fit.  The powers are computed in float64 on the device and rounded once to float32; the
walk adds float32 products in a fixed order, so two fits give the same bits.  ``predict`` / ``rank`` / ``full_rank`` /
``full_rank_users`` / ``full_rank_positions`` / ``w_sparse`` / ``pred_mat`` are ItemKNNCF's.  There is no CPU path.

``fit(train_set)`` takes the training DataFrame exactly as ``ItemKNNCF.fit`` does (columns ``user`` / ``item`` /
``rating``); duplicate (user, item) pairs are summed (one interaction when ``implicit``).
"""
from __future__ import annotations

import math

import torch

from .. import ops
from .AbstractRecommender import GeneralRecommender
from .KNNCFRecommender import _KNNCF


class RP3beta(_KNNCF):
    _name = "RP3beta"

    def __init__(self, config):
        """Config keys: user_num, item_num, topk; maxk (100): the entries kept per row of W; alpha (1.0); beta (0.6);
        implicit (True): every stored value becomes 1; normalize_similarity (False): every row of W divided by its
        sum; gpu, logger."""
        GeneralRecommender.__init__(self, config)
        self.user_num = int(config["user_num"])
        self.item_num = int(config["item_num"])
        self.topk = int(config["topk"])
        self.k = int(config.get("maxk", 100))
        self.alpha = float(config.get("alpha", 1.0))
        self.beta = self._beta_of(config)
        self.implicit = bool(config.get("implicit", True))
        self.normalize_similarity = bool(config.get("normalize_similarity", False))
        for name, v in (("alpha", self.alpha), ("beta", self.beta)):
            if not v >= 0 or not math.isfinite(v):
                raise ValueError(f"{self._name}: {name}={v} must be >= 0 and finite")
        if self.k < 1:
            raise ValueError(f"{self._name}: maxk={self.k} must be >= 1")
        if self.topk < 1:
            raise ValueError(f"{self._name}: topk={self.topk} must be >= 1")
        if self.user_num < 1 or self.item_num < 1:
            raise ValueError(f"{self._name}: user_num={self.user_num}, item_num={self.item_num} must be positive")
        self._csr = self._csr_t = self._W = self._L = self._R = None
        self._inner = self.item_num
        self._P = None
        self.scales = None          # (user_scale [U], item_scale [I], col_scale [I]) float32 on the device, after fit
        self.fit_info = None

    @staticmethod
    def _beta_of(config):
        return float(config.get("beta", 0.6))

    @staticmethod
    def _powers(csr, rows, alpha):
        """(the CSR with the values x^alpha * s, the scale s = (row sum)^-alpha per row [0 for an empty row]): the powers
        and their product in float64, rounded once to float32 (with values of 1 an entry IS its row's scale)"""
        row_ptr, col, val = csr
        lens = row_ptr[1:] - row_ptr[:-1]
        rowid = torch.repeat_interleave(torch.arange(rows, device=val.device), lens)
        x = val.to(torch.float64)
        total = torch.segment_reduce(x, "sum", lengths=lens)          # every row's entries in stored order: no atomics
        scale = torch.where(total > 0, total.clamp_min(1e-300).pow(-alpha), torch.zeros_like(total))
        p = x.pow(alpha) * scale[rowid]
        return (row_ptr, col, p.to(torch.float32).contiguous()), scale.to(torch.float32)

    def _frame_columns(self, df):
        users, items, ratings = super()._frame_columns(df)
        if not self.implicit and ratings.size and ratings.min() <= 0:
            raise ValueError(f"{self._name}.fit: column 'rating' holds {ratings.min()}: a transition probability needs "
                             "ratings > 0 (implicit=True takes every stored pair as 1)")
        return users, items, ratings

    def fit(self, train_set):
        csr, csr_t = self._frame_csr(train_set, transposed=True)
        if self.implicit:
            csr, csr_t = ((c[0], c[1], torch.ones_like(c[2])) for c in (csr, csr_t))
        n = self.item_num
        k = min(self.k, n)
        if k > ops.N.KNN_MAX_K:
            raise ValueError(f"{self._name}: min(maxk, item_num)={k} above {ops.N.KNN_MAX_K}")
        Pui, user_scale = self._powers(csr, self.user_num, self.alpha)
        Piu, item_scale = self._powers(csr_t, n, self.alpha)
        deg = (csr_t[0][1:] - csr_t[0][:-1]).to(torch.float64)                   # the users of every item
        col_scale = torch.where(deg > 0, deg.clamp_min(1.0).pow(-self.beta), torch.zeros_like(deg)).to(torch.float32)
        self._W = None
        count, cols, vals = ops.walk2_topk(Piu, Pui, n, k, col_scale, zero_diagonal=True,
                                           normalize=self.normalize_similarity, validate=False)
        W = ops.knn_rows_of_columns(ops.slim_columns(count, cols, vals, n), n)  # by row -> by column: knn_rank's R
        self._csr, self._csr_t, self._W = csr, csr_t, W
        self._L, self._R, self._inner = csr, W, n
        self.scales = (user_scale, item_scale, col_scale)
        self._P = (Piu, Pui)        # the operands of the walk (they share X's pattern)
        user_deg = (csr[0][1:] - csr[0][:-1])
        held = sum(t.numel() * t.element_size() for t in csr + csr_t + W + self.scales + (Piu[2], Pui[2]))
        self.fit_info = {"n": n, "nnz": int(W[0][-1].item()), "bytes_held": held, "paths": int((user_deg * user_deg).sum().item())}


class P3alpha(RP3beta):
    """RP3beta without the popularity penalty (beta = 0)."""
    _name = "P3alpha"

    @staticmethod
    def _beta_of(config):
        return 0.0
