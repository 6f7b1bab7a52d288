"""EASE (embarrassingly shallow auto-encoder) with the reference's interface, fitted by HIP kernels.

Mirror of daisy/model/EASERecommender.py (class ``EASE``): same config keys (``reg``, ``topk``, ``user_num``,
``item_num`` and the column names ``UID_NAME`` / ``IID_NAME`` / ``INTER_NAME``), ``fit(train_set)`` takes the training
DataFrame, ``predict`` / ``rank`` / ``full_rank`` return the reference's types, ``item_similarity`` and
``interaction_matrix`` are the reference's arrays.  The reference inverts ``X^T X + reg I`` with ``np.linalg.inv``; here the
Gram matrix comes from the fp32 MFMA product (``daisy_slim_gram``), the inverse from a blocked fp64 Cholesky
factorisation on the fp64 MFMA (``daisy_ease_potrf`` / ``daisy_ease_potri``) and the scores ``X[u, :] B`` are computed per
request from the user's CSR row (``daisy_ease_rank``).  There is no CPU path.

Deviations: ``reg`` must be positive (the reference accepts ``reg <= 0`` and then inverts a matrix that is
singular whenever an item is unrated); the ratings pass through fp32 in the CSR (as in the reference's ``astype``); ties
are ranked in stable order where the reference's argsort leaves them unspecified - a user without history scores exactly
0 everywhere and gets the first ``topk`` candidates; ``rank`` orders the candidates by the scores of ``predict`` and
``full_rank`` (``X[u, :] B[:, c]``), where the reference's ``rank`` reads ``B`` transposed (EASERecommender.py:60).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .AbstractRecommender import GeneralRecommender


class EASE(GeneralRecommender):
    def __init__(self, config):
        """Config keys as in EASERecommender.py:17-28 (ease.yaml + basic.yaml)."""
        super().__init__(config)
        self.inter_name = config["INTER_NAME"]
        self.iid_name = config["IID_NAME"]
        self.uid_name = config["UID_NAME"]
        self.user_num = int(config["user_num"])
        self.item_num = int(config["item_num"])
        self.reg_weight = float(config["reg"])
        self.topk = int(config["topk"])
        if not self.reg_weight > 0 or not np.isfinite(self.reg_weight):
            raise ValueError(f"EASE: reg={self.reg_weight} must be positive and finite (X^T X alone is singular whenever an "
                             "item is unrated)")
        if self.topk < 1:
            raise ValueError(f"EASE: topk={self.topk} must be >= 1")
        if self.user_num < 1 or self.item_num < 1:
            raise ValueError(f"EASE: user_num={self.user_num}, item_num={self.item_num} must be positive")
        self._csr = None            # X on the device
        self._B = None              # float64 [item_num, item_num] on the device
        self.fit_info = None

    # -- fit -----------------------------------------------------------------------------------------------------------
    def _frame_columns(self, df):
        """EASERecommender.py:31-33: the configured columns, range-checked."""
        cols = []
        for name, hi, what in ((self.uid_name, self.user_num, "user"), (self.iid_name, self.item_num, "item")):
            ids = np.asarray(df[name])
            if ids.size and not np.issubdtype(ids.dtype, np.integer):
                if not np.all(ids == np.floor(ids)):
                    raise ValueError(f"EASE.fit: column '{name}' holds non-integer ids")
            ids = ids.astype(np.int64)
            if ids.size and (ids.min() < 0 or ids.max() >= hi):
                bad = ids.max() if ids.max() >= hi else ids.min()
                raise ValueError(f"EASE.fit: {what} id {int(bad)} outside [0, {hi})")
            cols.append(ids)
        ratings = np.asarray(df[self.inter_name], dtype=np.float64)
        if not np.all(np.isfinite(ratings)):
            raise ValueError(f"EASE.fit: column '{self.inter_name}' holds a value that is not finite")
        return cols[0], cols[1], ratings

    def fit(self, train_set):
        """EASERecommender.py:30-47: Gram matrix, the fp64 inverse, B = -P / diag(P); B and X stay on the device."""
        users, items, ratings = self._frame_columns(train_set)
        self._require_device()
        dev = torch.device(self.device)
        csr = ops.slim_csr(torch.from_numpy(users).to(dev), torch.from_numpy(items).to(dev),
                           torch.from_numpy(ratings).to(dev), self.user_num, self.item_num)
        B, info = ops.ease_fit(csr, self.item_num, self.reg_weight)
        info = int(info.cpu().item())
        self.fit_info = {"info": info, "bytes_held": B.numel() * 8 + sum(t.numel() * t.element_size() for t in csr),
                         "bytes_peak": int(ops.lib.daisy_ease_fit_bytes(self.item_num))}
        if info != 0:
            raise RuntimeError(f"EASE.fit: X^T X + {self.reg_weight} I is not positive definite: the Cholesky pivot of "
                               f"column {info - 1} is not positive")
        self._csr, self._B = csr, B

    def _fitted(self):
        self._require_device()
        if self._B is None:
            raise RuntimeError("EASE: fit(train_set) has not been called")

    # -- the reference's attributes, built on demand -------------------------------------------------------------------
    @property
    def item_similarity(self):
        """EASERecommender.py:45-46: numpy float64 [item_num, item_num]; None before fit."""
        return None if self._B is None else self._B.cpu().numpy()

    @property
    def interaction_matrix(self):
        """EASERecommender.py:47: scipy.sparse.csr_matrix float32 [user_num, item_num]; None before fit."""
        if self._csr is None:
            return None
        import scipy.sparse as sp
        row_ptr, col, val = (t.cpu().numpy() for t in self._csr)
        nnz = int(row_ptr[-1])
        return sp.csr_matrix((val[:nnz], col[:nnz], row_ptr), shape=(self.user_num, self.item_num), dtype=np.float32)

    # -- scores --------------------------------------------------------------------------------------------------------
    def _check(self, ids, hi, what):
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= hi):
            raise IndexError(f"index out of range: {what} ids must lie in [0, {hi})")

    def _rank(self, users, items=None, topk=0):
        self._fitted()
        users = torch.as_tensor(users).reshape(-1).to(self.device, torch.int64)
        self._check(users, self.user_num, "user")
        if items is not None:
            items = torch.as_tensor(items).to(self.device, torch.int64)
            self._check(items, self.item_num, "item")
        return ops.ease_rank(self._csr, self._B, users, items, topk)

    def predict(self, u, i):
        """EASERecommender.py:49-50 -> one float."""
        return float(self._rank([int(u)], torch.tensor([[int(i)]], dtype=torch.int64))[0].cpu().item())

    def rank(self, test_loader):
        """EASERecommender.py:52-67 -> the candidates' ids int64 [n_users, topk], best first by predict's scores (the
        reference's line 60 gathers B's rows where predict reads its columns: DESIGN.md §17)."""
        self._fitted()
        out = self._rank_loader(test_loader, lambda us, cands_ids: self._rank(us, cands_ids, self.topk)[1])
        return out.astype(np.int64)                                  # (the reference returns the int64 ids)

    def full_rank(self, u):
        """EASERecommender.py:69-71 -> int64 [topk] over all items."""
        return self._rank([int(u)], None, self.topk)[1].view(-1).cpu().numpy()

    def full_rank_users(self, users, exclude=None, return_scores=False):
        """Full ranking of many users in one launch (no counterpart in the reference): device int64
        [len(users), topk], row b = full_rank(users[b]) without the items of the user's row of `exclude` (None, an
        (indptr, items) device CSR or a train_ur dict of sets); -1 where a user has fewer eligible items than topk.
        return_scores: (ids, float64 scores)."""
        self._fitted()
        users, exclude = self._users_and_exclusion(users, exclude, self.user_num, self.device)
        return ops.ease_full_rank_users(self._csr, self._B, users, self.topk, exclude=exclude, return_scores=return_scores)
