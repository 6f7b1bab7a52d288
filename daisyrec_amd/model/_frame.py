"""What the models fitted from a training DataFrame share: the checked columns of the frame, and `FrameRecommender`, the
base of the families whose scores are a fixed-order sum over sparse or dense fp64 operands (EASE, SLiM, ItemKNNCF /
UserKNNCF / RP3beta / P3alpha, PureSVD).  A family supplies its fit, the tuple of operands its `ops`
functions take (`_operands`) and those functions (`_rank_op`, `_users_op`, `_positions_op`); the request handling, the
range checks and the five ranking entry points are written once here.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .AbstractRecommender import GeneralRecommender


def id_column(df, column, hi, who, what):
    """df[column] as int64 ids in [0, hi); ValueError in the name of `who` for a value that is no integer or lies outside
    (a float column holding whole numbers is taken)."""
    ids = np.asarray(df[column])
    if ids.size and not np.issubdtype(ids.dtype, np.integer):
        if not np.all(ids == np.floor(ids)):
            raise ValueError(f"{who}.fit: column '{column}' holds non-integer ids")
    ids = ids.astype(np.int64)
    if ids.size and (ids.min() < 0 or ids.max() >= hi):
        bad = ids.max() if ids.max() >= hi else ids.min()
        raise ValueError(f"{who}.fit: {what} id {int(bad)} outside [0, {hi})")
    return ids


def frame_columns(df, columns, user_num, item_num, who):
    """(users int64, items int64, ratings float64) of the three `columns` (user, item, rating) of df: the ids
    range-checked, the ratings finite."""
    uid, iid, inter = columns
    users = id_column(df, uid, user_num, who, "user")
    items = id_column(df, iid, item_num, who, "item")
    ratings = np.asarray(df[inter], dtype=np.float64)
    if not np.all(np.isfinite(ratings)):
        raise ValueError(f"{who}.fit: column '{inter}' holds a value that is not finite")
    return users, items, ratings


class FrameRecommender(GeneralRecommender):
    _name = None                                # the class's name in its messages
    _columns = ("user", "item", "rating")       # the frame's columns (the reference hard-codes them; EASE configures them)
    # ops.<family>_rank, ops.<family>_full_rank_users, ops.<family>_full_rank_positions, called on (*_operands(), ...);
    # a class without _positions_op has no full_rank_positions
    _rank_op = _users_op = _positions_op = None

    def _operands(self):
        """the leading arguments of the family's ops functions"""
        raise NotImplementedError

    def _has_fit(self):
        raise NotImplementedError

    # -- fit -----------------------------------------------------------------------------------------------------------
    def _frame_columns(self, df):
        return frame_columns(df, self._columns, self.user_num, self.item_num, self._name)

    def _frame_csr(self, train_set, transposed=False):
        """(X, X^T or None) as ops.slim_csr's triples on the device.  The frame is checked before the device is: a bad
        frame raises its ValueError on a host without one too."""
        users, items, ratings = self._frame_columns(train_set)
        self._require_device()
        dev = torch.device(self.device)
        u, i, r = (torch.from_numpy(a).to(dev) for a in (users, items, ratings))
        csr = ops.slim_csr(u, i, r, self.user_num, self.item_num)
        return csr, (ops.slim_csr(i, u, r, self.item_num, self.user_num) if transposed else None)

    def _fitted(self):
        self._require_device()
        if not self._has_fit():
            raise RuntimeError(f"{self._name}: fit(train_set) has not been called")

    # -- scores --------------------------------------------------------------------------------------------------------
    def _check(self, ids, hi, what):
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= hi):
            raise IndexError(f"index out of range: {what} ids must lie in [0, {hi})")

    def _request(self, users, items):
        """(users int64 [B], items int64 or None) on the device, range-checked, of a fitted model"""
        self._fitted()
        users = torch.as_tensor(users).reshape(-1).to(self.device, torch.int64)
        self._check(users, self.user_num, "user")
        if items is not None:
            items = torch.as_tensor(items).to(self.device, torch.int64)
            self._check(items, self.item_num, "item")
        return users, items

    def _rank(self, users, items=None, topk=0):
        """(float64 scores [B, C], ids int64 [B, min(topk, C)] or None) of users [B] at the candidates items [B, C]
        (None: every item)"""
        users, items = self._request(users, items)
        return self._rank_op(*self._operands(), users, items, topk)

    def predict(self, u, i):
        """-> one float, as the reference's predict"""
        return float(self._rank([int(u)], torch.tensor([[int(i)]], dtype=torch.int64))[0].cpu().item())

    def rank(self, test_loader):
        """-> the candidates' ids int64 [n_users, topk], best first by predict's scores (shape (0,) for an empty loader)"""
        self._fitted()
        out = self._rank_loader(test_loader, lambda us, cands_ids: self._rank(us, cands_ids, self.topk)[1])
        return out.astype(np.int64)             # _rank_loader hands the ids over as float32: exact only for ids below 2^24

    def full_rank(self, u):
        """-> int64 [topk] over all items"""
        return self._rank([int(u)], None, self.topk)[1].view(-1).cpu().numpy()

    def full_rank_users(self, users, exclude=None, return_scores=False):
        """Full ranking of many users in one launch (no counterpart in the reference): device int64
        [len(users), topk], row b = full_rank(users[b]) without the items of the user's row of `exclude` (None, an
        (indptr, items) device CSR or a train_ur dict of sets); -1 where a user has fewer eligible items than topk.
        return_scores: (ids, scores) - float32 scores for SLiM (its float64 sums rounded once, which it ranks by),
        float64 for EASE, ItemKNNCF, UserKNNCF, RP3beta, P3alpha and PureSVD."""
        self._fitted()
        users, exclude = self._users_and_exclusion(users, exclude, self.user_num, self.device)
        return self._users_op(*self._operands(), users, self.topk, exclude=exclude, return_scores=return_scores)

    def full_rank_positions(self, users, targets, exclude=None, **kw):
        """The exact rank of every held-out item among all eligible items, in one launch (no counterpart in the
        reference): `targets` and `exclude` are an (indptr, items) device CSR or a dict of sets (test_ur /
        train_ur); -> ops.full_rank_positions' tuple, consistent with full_rank_users - its ids[b, pos] is the target
        wherever pos < topk - without the cap on topk.  kw: return_scores (float32 for SLiM, float64 for the others, as
        full_rank_users), return_eligible, validate, and path where the family's ops function takes one (not PureSVD)."""
        if self._positions_op is None:
            return super().full_rank_positions(users, targets, exclude, **kw)
        self._fitted()
        users, exclude = self._users_and_exclusion(users, exclude, self.user_num, self.device)
        _, targets = self._users_and_exclusion(users, targets, self.user_num, self.device)
        return self._positions_op(*self._operands(), users, targets, exclude=exclude, **kw)
