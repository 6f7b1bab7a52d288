"""MostPop with the reference's interface, counted and ranked by HIP kernels.

Mirror of daisy/model/PopRecommender.py (class ``MostPop``): same config keys (``item_num``, ``topk``, ``IID_NAME``),
``fit(train_set)`` takes the training DataFrame and counts its item column, ``predict`` / ``rank`` / ``full_rank`` return
the reference's types, ``item_cnt_ref`` and ``item_score`` are the reference's float64 arrays, fetched on demand.  The
counts come from integer atomics (``daisy_pop_fit``), ``item_score = cnt / (1 + cnt)`` is the reference's one float64
division and has its bits; ``rank`` gathers the candidates' scores and takes the shared fp64 top-k (``daisy_pop_rank``).
There is no CPU path.

Deviations: ids outside ``[0, item_num)`` and non-integer ids in the item column raise ``ValueError``
(the reference's fancy assignment raises ``IndexError`` or wraps a negative id around); equal scores are ordered by
candidate position in ``rank`` and by item id in ``full_rank`` (the reference's ``torch.argsort`` / ``np.argsort`` leave
ties open).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .AbstractRecommender import GeneralRecommender
from ._frame import id_column


class MostPop(GeneralRecommender):
    def __init__(self, config):
        """Config keys as in PopRecommender.py:17-27."""
        super().__init__(config)
        self.item_num = int(config["item_num"])
        self.topk = int(config["topk"])
        self.cnt_col = config["IID_NAME"]
        if self.item_num < 1:
            raise ValueError(f"MostPop: item_num={self.item_num} must be positive")
        if self.topk < 1:
            raise ValueError(f"MostPop: topk={self.topk} must be >= 1")
        self._cnt = self._score = None
        self._full = None           # full_rank's list: the same for every user

    def fit(self, train_set):
        """PopRecommender.py:30-33: the counts of the column config['IID_NAME'], range-checked."""
        ids = id_column(train_set, self.cnt_col, self.item_num, "MostPop", self.cnt_col)
        self._require_device()
        self._cnt, self._score = ops.pop_fit(torch.from_numpy(ids).to(self.device), self.item_num)
        self._full = None

    def _fitted(self):
        self._require_device()
        if self._score is None:
            raise RuntimeError("MostPop: fit(train_set) has not been called")

    @property
    def item_cnt_ref(self):
        """PopRecommender.py:25, 32: float64 [item_num] (zeros before fit)"""
        if self._cnt is None:
            return np.zeros(self.item_num)
        return self._cnt.cpu().numpy().astype(np.float64)

    @property
    def item_score(self):
        """PopRecommender.py:33: float64 [item_num]; None before fit"""
        return None if self._score is None else self._score.cpu().numpy()

    def predict(self, u, i):
        """PopRecommender.py:35-36 -> item_score[i]"""
        self._fitted()
        i = int(i)
        if not 0 <= i < self.item_num:
            raise IndexError(f"index out of range: item ids must lie in [0, {self.item_num})")
        return np.float64(self._score[i].cpu().item())

    def _topk(self, us, cands_ids):
        cands_ids = cands_ids.to(torch.int64)
        if cands_ids.numel() and (int(cands_ids.min()) < 0 or int(cands_ids.max()) >= self.item_num):
            raise IndexError(f"index out of range: item ids must lie in [0, {self.item_num})")
        return ops.pop_rank(self._score, cands_ids, self.topk)

    def rank(self, test_loader):
        """PopRecommender.py:38-51 -> the candidates' ids float32 [n_users, topk], best first."""
        self._fitted()
        return self._rank_loader(test_loader, self._topk)

    def full_rank(self, u):
        """PopRecommender.py:53-54 -> int64 [topk] over all items (the same for every user: computed once per fit)."""
        self._fitted()
        if self._full is None:
            self._full = ops.pop_rank(self._score, None, self.topk).view(-1).cpu().numpy()
        return self._full.copy()
