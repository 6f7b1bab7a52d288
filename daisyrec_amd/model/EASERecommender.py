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

from .. import ops
from ._frame import FrameRecommender


class EASE(FrameRecommender):
    _name = "EASE"
    _rank_op = staticmethod(ops.ease_rank)
    _users_op = staticmethod(ops.ease_full_rank_users)      # (no _positions_op yet: ops.ease_full_rank_positions is there)

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
    @property
    def _columns(self):
        """EASERecommender.py:31-33: the configured columns"""
        return self.uid_name, self.iid_name, self.inter_name

    def fit(self, train_set):
        """EASERecommender.py:30-47: Gram matrix, the fp64 inverse, B = -P / diag(P); B and X stay on the device."""
        csr, _ = self._frame_csr(train_set)
        B, info = ops.ease_fit(csr, self.item_num, self.reg_weight)
        info = int(info.cpu().item())
        self.fit_info = {"info": info, "bytes_held": B.numel() * 8 + sum(t.numel() * t.element_size() for t in csr),
                         "bytes_peak": int(ops.lib.daisy_ease_fit_bytes(self.item_num))}
        if info != 0:
            raise RuntimeError(f"EASE.fit: X^T X + {self.reg_weight} I is not positive definite: the Cholesky pivot of "
                               f"column {info - 1} is not positive")
        self._csr, self._B = csr, B

    def _has_fit(self):
        return self._B is not None

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

    # -- scores: FrameRecommender's, on X[u, :] B (EASERecommender.py:49-71; rank orders the candidates by predict's scores,
    # where the reference's line 60 gathers B's rows: DESIGN.md §17) -------------------------------------------------------
    def _operands(self):
        return self._csr, self._B
