"""PureSVD with the reference's interface, fitted by HIP kernels.

Mirror of daisy/model/PureSVDRecommender.py (class ``PureSVD``): same config keys (``user_num``, ``item_num``,
``factors``, ``topk``), ``fit(train_set)`` takes the training DataFrame, ``predict`` / ``rank`` / ``full_rank`` return the
reference's types, ``user_vec`` / ``item_vec`` are the reference's arrays.  The reference calls scikit-learn's
``randomized_svd(X, n_components=factors, random_state=2019)``, whose result is NOT the truncated SVD but a deterministic
function of a random test matrix; here the same sequence runs in fp64 on the device (``ops.psvd_fit``: sparse x
tall-skinny products, Cholesky-QR2 orthonormalisation on the fp64 MFMA, one small Jacobi SVD) from the same test matrix,
which is drawn on the host exactly as scikit-learn draws it.  There is no CPU path.

Deviations: the range finder is normalised by Cholesky-QR2 instead of LU (only the span matters); the
ratings pass through fp32 in the CSR (exact for the integer and half-step ratings the loaders produce); ties are ranked
in stable order where the reference's argsort leaves them unspecified.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .. import _native as N
from ._frame import FrameRecommender

_OVERSAMPLES = 10          # randomized_svd's n_oversamples
_SEED = 2019               # PureSVDRecommender.py:44


class PureSVD(FrameRecommender):
    _name = "PureSVD"
    _rank_op = staticmethod(ops.psvd_rank)
    _users_op = staticmethod(ops.psvd_full_rank_users)
    _positions_op = staticmethod(ops.psvd_full_rank_positions)

    def __init__(self, config):
        """Config keys as in PureSVDRecommender.py:28-36 (puresvd.yaml + basic.yaml); ``puresvd_max_sweeps`` (60) bounds
        the Jacobi sweeps of the small SVD."""
        super().__init__(config)
        self.user_num = int(config["user_num"])
        self.item_num = int(config["item_num"])
        self.factors = int(config["factors"])
        self.topk = int(config["topk"])
        self.max_sweeps = int(config.get("puresvd_max_sweeps", 60))
        if self.factors < 1:
            raise ValueError(f"PureSVD: factors={self.factors} must be >= 1")
        if self.factors + _OVERSAMPLES > N.PSVD_MAX_C:
            raise ValueError(f"PureSVD: factors={self.factors} + {_OVERSAMPLES} oversamples exceed the {N.PSVD_MAX_C} "
                             "columns the kernels hold")
        if self.topk < 1:
            raise ValueError(f"PureSVD: topk={self.topk} must be >= 1")
        if self.user_num < 1 or self.item_num < 1:
            raise ValueError(f"PureSVD: user_num={self.user_num}, item_num={self.item_num} must be positive")
        self._user_vec = None       # float64 [user_num, factors] on the device
        self._item_vec = None       # float64 [item_num, factors] on the device
        self.fit_info = None
        self.logger.info(f"user num: {self.user_num}, item num: {self.item_num}")

    # -- fit -----------------------------------------------------------------------------------------------------------
    def fit(self, train_set):
        """PureSVDRecommender.py:38-49: randomized_svd of the rating matrix; user_vec = U, item_vec = V diag(sigma).
        The frame's columns are 'user', 'item', 'rating' (PureSVDRecommender.py:51-58 hard-codes them)."""
        x, xt = self._frame_csr(train_set, transposed=True)
        self.logger.info("Computing SVD decomposition...")
        self.logger.info('Finish build train matrix for decomposition')
        dev = torch.device(self.device)
        U, I, k = self.user_num, self.item_num, self.factors
        transposed = U < I                                            # randomized_svd: transpose='auto'
        n_iter = 7 if k < 0.1 * min(U, I) else 4                      # randomized_svd: n_iter='auto'
        m_csr, mt_csr, m = (xt, x, U) if transposed else (x, xt, I)   # M [n, m], n >= m
        omega = np.random.RandomState(_SEED).normal(size=(m, k + _OVERSAMPLES))
        left, s, right, dropped, info = ops.psvd_fit(m_csr, mt_csr, torch.from_numpy(omega).to(dev), n_iter, self.max_sweeps)
        user_side, item_side = (right, left) if transposed else (left, right)
        # svd_flip: in both orientations the sign comes from the largest-|.| entry of a component's user-side vector
        top = torch.argmax(user_side.abs(), dim=0, keepdim=True)
        sign = torch.sign(torch.gather(user_side, 0, top))
        self._user_vec = (user_side * sign)[:, :k].contiguous()
        self._item_vec = ((item_side * sign)[:, :k] * s[:k]).contiguous()
        status, sweeps = (int(v) for v in info.cpu())
        self.fit_info = {"n_iter": n_iter, "transposed": transposed, "dropped": [int(d) for d in dropped.cpu()],
                         "sigma": s[:k].cpu().numpy(), "jacobi_sweeps": sweeps}
        if status != N.PSVD_CONVERGED:
            raise RuntimeError(f"PureSVD.fit: the Jacobi SVD did not converge in {self.max_sweeps} sweeps "
                               "(config['puresvd_max_sweeps'])")
        self.logger.info('Done!')

    def _has_fit(self):
        return self._user_vec is not None

    # -- the reference's attributes, fetched on access -----------------------------------------------------------------
    @property
    def user_vec(self):
        """PureSVDRecommender.py:47: float64 [user_num, factors]; None before fit."""
        return None if self._user_vec is None else self._user_vec.cpu().numpy()

    @property
    def item_vec(self):
        """PureSVDRecommender.py:48: float64 [item_num, factors] (V diag(sigma)); None before fit."""
        return None if self._item_vec is None else self._item_vec.cpu().numpy()

    # -- scores: FrameRecommender's, on <user_vec[u], item_vec[i]> (PureSVDRecommender.py:60-83) ------------------------
    def _operands(self):
        return self._user_vec, self._item_vec

    def rank(self, test_loader):
        """PureSVDRecommender.py:63-78 -> the candidates' ids int64 [n_users, topk], best first ((0, topk) for an empty
        loader)."""
        self._fitted()
        out = []
        for us, cands_ids in test_loader:                 # (not _rank_loader: it returns float32, the reference int64)
            cands_ids = torch.as_tensor(cands_ids)
            if cands_ids.dim() == 1:
                cands_ids = cands_ids.unsqueeze(0)
            out.append(self._rank(us, cands_ids, self.topk)[1])
        if not out:
            return np.zeros((0, self.topk), dtype=np.int64)
        return torch.cat(out, 0).cpu().numpy()
