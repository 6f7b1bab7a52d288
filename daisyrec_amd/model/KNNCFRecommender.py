"""ItemKNN and UserKNN with the reference's interface, fitted by HIP kernels.

Mirror of daisy/model/KNNCFRecommender.py (classes ``ItemKNNCF`` and ``UserKNNCF``): same config keys (``maxk``,
``shrink``, ``normalize``, ``similarity``, ``topk``, ``user_num``, ``item_num``), ``fit(train_set)`` takes the training
DataFrame and reads its columns ``user`` / ``item`` / ``rating`` (the reference's ``convert_df`` names them literally),
``predict`` / ``rank`` / ``full_rank`` return the reference's types and ``pred_mat`` is the reference's scipy matrix, built
on demand.  The similarity of the columns of D (X for ItemKNN, X^T for UserKNN) comes from the Gram matrix on the fp32
MFMA product (``daisy_slim_gram``), the reference's fp32 weight formula and a radix select of every column's ``maxk``
largest weights (``daisy_knn_select``); the fp64 scores ``X W`` / ``W X`` are computed per request from the two sparse
operands (``daisy_knn_rank``).  There is no CPU path.

Deviations: the ratings pass through fp32 in the CSR (the reference keeps the DataFrame's float64 in the
product ``train.dot(w_sparse)``; integer ratings are unaffected); ``shrink < 0`` is refused; ties are ordered where the
reference leaves them open - among equal weights at the boundary of a column's ``maxk`` largest the LOWER row is kept
(the reference keeps whatever ``argpartition`` leaves), and ``rank`` / ``full_rank`` order equal scores by position (the
reference's ``argsort`` is unstable): a user without history scores exactly 0 everywhere and gets the first ``topk``
candidates.
"""
from __future__ import annotations

import numpy as np

from .. import ops
from ._frame import FrameRecommender


class _KNNCF(FrameRecommender):
    _name = "KNNCF"
    _rank_op = staticmethod(ops.knn_rank)
    _users_op = staticmethod(ops.knn_full_rank_users)
    _positions_op = staticmethod(ops.knn_full_rank_positions)

    def __init__(self, config):
        """Config keys as in KNNCFRecommender.py:402-413 / :481-491 (itemknn.yaml + basic.yaml)."""
        super().__init__(config)
        self.user_num = int(config["user_num"])
        self.item_num = int(config["item_num"])
        self.k = int(config["maxk"])
        self.shrink = float(config["shrink"])
        self.normalize = bool(config["normalize"])
        self.similarity = config["similarity"]
        self.topk = int(config["topk"])
        ops.knn_plan(self.similarity, self.normalize)                # the reference's ValueError for an unknown name
        if not (self.shrink >= 0 and np.isfinite(self.shrink)):
            raise ValueError(f"{self._name}: shrink={self.shrink} must be finite and >= 0")
        if self.k < 1:
            raise ValueError(f"{self._name}: maxk={self.k} must be >= 1")
        if self.topk < 1:
            raise ValueError(f"{self._name}: topk={self.topk} must be >= 1")
        if self.user_num < 1 or self.item_num < 1:
            raise ValueError(f"{self._name}: user_num={self.user_num}, item_num={self.item_num} must be positive")
        self._csr = None            # X by row on the device
        self._csr_t = None          # X by column (the CSR of X^T)
        self._W = None              # the similarity by column: (ptr, row, val)
        self._L = self._R = None    # the operands of the score product
        self.fit_info = None

    # -- fit -----------------------------------------------------------------------------------------------------------
    def _similarity_of(self, csr, csr_t):
        raise NotImplementedError

    def fit(self, train_set):
        """The frame's columns are 'user', 'item', 'rating' (KNNCFRecommender.py:36-38 names them literally)."""
        csr, csr_t = self._frame_csr(train_set, transposed=True)
        self._W = None
        W, n, rows_d = self._similarity_of(csr, csr_t)
        self._csr, self._csr_t, self._W = csr, csr_t, W
        held = sum(t.numel() * t.element_size() for t in csr + csr_t + W)
        if self._L is not csr:
            held += sum(t.numel() * t.element_size() for t in self._L)
        self.fit_info = {"n": n, "nnz": int(W[0][-1].item()), "bytes_held": held,
                         "bytes_peak": int(ops.lib.daisy_knn_fit_bytes(rows_d, n, min(self.k, n)))}

    def _knn(self, csr_D, csr_Dt, n):
        k = min(self.k, n)                                           # KNNCFRecommender.py:114
        if k > ops.N.KNN_MAX_K:
            raise ValueError(f"{self._name}: min(maxk, n)={k} above {ops.N.KNN_MAX_K}")
        return ops.knn_fit(csr_D, n, self.similarity, self.shrink, k, normalize=self.normalize, csr_Dt=csr_Dt)

    def _has_fit(self):
        return self._W is not None

    # -- the reference's attributes, built on demand -------------------------------------------------------------------
    @property
    def w_sparse(self):
        """The similarity matrix, scipy.sparse.csc_matrix float32 [n, n]; None before fit."""
        if self._W is None:
            return None
        import scipy.sparse as sp
        ptr, row, val = (t.cpu().numpy() for t in self._W)
        nnz, n = int(ptr[-1]), len(ptr) - 1
        return sp.csc_matrix((val[:nnz], row[:nnz], ptr), shape=(n, n), dtype=np.float32)

    @property
    def pred_mat(self):
        """KNNCFRecommender.py:432 / :510: scipy.sparse.lil_matrix float64 [user_num, item_num]; None before fit."""
        if self._W is None:
            return None
        import scipy.sparse as sp
        full = self._rank(np.arange(self.user_num), None, 0)[0].cpu().numpy()
        return sp.csr_matrix(full).tolil()

    # -- scores: FrameRecommender's, on L[u, :] R (KNNCFRecommender.py:434-457) -----------------------------------------
    def _operands(self):
        return self._L, self._R, self._inner, self.item_num


class ItemKNNCF(_KNNCF):
    """pred_mat = X W, W the similarity of X's columns (KNNCFRecommender.py:380-457)."""
    _name = "ItemKNNCF"

    def _similarity_of(self, csr, csr_t):
        W = self._knn(csr, csr_t, self.item_num)
        self._L, self._R, self._inner = csr, W, self.item_num
        return W, self.item_num, self.user_num


class UserKNNCF(_KNNCF):
    """pred_mat = W X, W the similarity of X^T's columns (KNNCFRecommender.py:459-535): score (u, c) sums over ROW u of W,
    which holds an entry for every v that keeps u among its neighbours - possibly more than maxk of them."""
    _name = "UserKNNCF"

    def _similarity_of(self, csr, csr_t):
        W = self._knn(csr_t, csr, self.user_num)
        self._L, self._R, self._inner = ops.knn_rows_of_columns(W, self.user_num), csr_t, self.user_num
        return W, self.user_num, self.item_num
