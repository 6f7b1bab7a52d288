"""The ranking KPIs of the reference on the device.

Mirror of daisy/utils/metrics.py: ``metrics_name_config``, ``calc_ranking_results(test_ur, pred_ur, test_u, config)``,
``Metric(config).run(...)`` and the functions ``Precision, Recall, MRR, MAP, NDCG, HR, AUC, F1, Coverage, Popularity,
Diversity`` with the reference's signatures and return types (a numpy float; a DataFrame with the columns ``'KPI@K'``, 1,
5, 10, ... for ``calc_ranking_results``).  Every one of them is ONE call of ``daisy_ranking_kpis`` (csrc/metrics.hip): a
wave per ranked list, all cutoffs and all requested KPIs from one pass over the lists, means summed in a fixed order, no
floating-point atomics - two calls give the same bits.  ``ranking_kpis`` is the device-native entry: it takes a prebuilt
device CSR of the truths (``utils.user_csr``) as well as the ``test_ur`` dict, whose conversion is a Python loop by the
dict's contract, and returns per-list values on request.  ``pred_ur`` may be float32 (what every ``rank`` returns),
int32 / int64 numpy, or a device tensor, which is used where it is.  There is no CPU path.

Deviations from the reference:
* ``Metric.run`` dispatches ``'f1'`` and ``'auc'`` on the metric's name; the reference tests ``kpi ==`` there
  (metrics.py:87-90) and reaches neither.
* ``item_pop`` is read when ``'popularity'`` is requested; the reference reads it only when ``'coverage'`` is
  (metrics.py:63) and hands Popularity ``None`` otherwise.
* ``'map'`` has a display name in ``metrics_name_config``.
* ids in ``pred_ur`` outside ``[0, item_num)``, non-integral float ids, a user of ``test_u`` without truths and
  ``i_categories`` that is not 0/1 raise ``ValueError`` (the reference computes something or fails later).
* popularity adds the distinct hit items in list order, diversity the pairs by their later member, the means by
  workgroup: the same terms as the reference in another order (bounds in DESIGN.md §20); everything that is one
  rounded operation on integers (precision, recall, hit, mrr, auc, coverage) has the reference's bits.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import ops
from .utils import _ur_pairs, user_csr

metrics_name_config = {
    "recall": 'Recall',
    "mrr": 'MRR',
    "ndcg": 'NDCG',
    "hit": 'Hit Ratio',
    "precision": 'Precision',
    "f1": 'F1-score',
    "auc": 'AUC',
    "coverage": 'Coverage',
    "diversity": 'Diversity',
    "popularity": 'Average Popularity',
    "map": 'MAP',
}

MAX_K = ops.N.METRICS_MAX_K


def _require_device():
    if not torch.cuda.is_available():
        raise RuntimeError("daisyrec_amd.utils.metrics needs a HIP device (no CPU fallback)")
    return torch.device("cuda")


def _check_names(metrics):
    for mc in metrics:
        if mc not in ops.N.KPI_IDS:
            raise ValueError(f'Invalid metric name {mc}')              # metrics.py:92


def _pred_ids(pred_ur, item_num):
    """pred_ur as int32 / int64 ids [n, K], range-checked: a numpy array is checked on the host (and stays there until
    the device is known to exist), a device tensor where it is."""
    if isinstance(pred_ur, torch.Tensor):
        t = pred_ur
        if t.dim() != 2:
            raise ValueError(f"pred_ur: expected [n_users, K], got {tuple(t.shape)}")
        if t.is_floating_point():
            if t.numel() and not bool((t == t.floor()).all()):
                raise ValueError("pred_ur holds non-integral ids")
            t = t.to(torch.int64)
        elif t.dtype not in (torch.int32, torch.int64):
            t = t.to(torch.int64)
        lo, hi = (int(t.min()), int(t.max())) if t.numel() else (0, 0)
    else:
        t = np.asarray(pred_ur)
        if t.ndim != 2:
            raise ValueError(f"pred_ur: expected [n_users, K], got {t.shape}")
        if not np.issubdtype(t.dtype, np.integer):
            if t.size and not np.all(t == np.floor(t)):
                raise ValueError("pred_ur holds non-integral ids")
            t = t.astype(np.int64)
        elif t.dtype not in (np.int32, np.int64):
            t = t.astype(np.int64)
        lo, hi = (int(t.min()), int(t.max())) if t.size else (0, 0)
    if t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"pred_ur: expected at least one list and one position, got {tuple(t.shape)}")
    if item_num is not None and (lo < 0 or hi >= item_num):
        raise ValueError(f"pred_ur: item id {lo if lo < 0 else hi} outside [0, {item_num})")
    if lo < 0:
        raise ValueError(f"pred_ur: item id {lo} is negative")
    return t, hi


def pack_categories(i_categories):
    """i_categories [item_num, C] with 0/1 entries -> (bit masks int64 [item_num, ceil(C / 64)] holding the uint64
    patterns - bit c of a row: the item has category c -, C)"""
    cats = np.asarray(i_categories)
    if cats.ndim != 2 or cats.shape[1] < 1:
        raise ValueError(f"i_categories: expected [item_num, category_num], got {cats.shape}")
    if not np.all((cats == 0) | (cats == 1)):
        raise ValueError("i_categories must hold 0/1 values")
    C = cats.shape[1]
    if C > ops.N.METRICS_MAX_CATS:
        raise ValueError(f"i_categories: {C} categories above {ops.N.METRICS_MAX_CATS}")
    W = (C + 63) // 64
    padded = np.zeros((cats.shape[0], W * 64), dtype=np.uint8)
    padded[:, :C] = cats.astype(np.uint8)
    bits = np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(cats.shape[0], W)
    return np.ascontiguousarray(bits).view(np.int64), C


def _truths(gt, test_u):
    """-> (pairs or a device CSR, max truth id or None); a user of test_u without truths is refused"""
    users = np.asarray(list(test_u) if not isinstance(test_u, (np.ndarray, torch.Tensor)) else
                       (test_u.cpu().numpy() if isinstance(test_u, torch.Tensor) else test_u)).astype(np.int64).reshape(-1)
    if isinstance(gt, (tuple, list)) and len(gt) == 2 and isinstance(gt[0], torch.Tensor):
        return gt, users, None
    for u in users.tolist():
        if u not in gt or len(gt[u]) == 0:
            raise ValueError(f"user {u} of test_u has no ground truth in test_ur")
    us, it = _ur_pairs(gt)
    return (us, it), users, (int(it.max()) if it.size else 0)


def ranking_kpis(pred, gt_csr_or_test_ur, test_u, cutoffs, metrics, item_num=None, item_pop=None, i_categories=None,
                 per_user=False):
    """Every KPI of `metrics` (names of metrics_name_config) at every cutoff (strictly ascending, <= pred.shape[1]) in one
    device call.  gt_csr_or_test_ur: the truths as {user: set(items)} or as the device CSR (indptr int64 [U + 1], items
    int32 ascending within a row) of utils.user_csr.  test_u: the owner of every list.  ->
    {'cutoffs': [...], 'means': {name: float64 [nc]}, 'per_user': {name: float64 [nc, n]} or None,
     'coverage_counts': int64 [nc] or None}; means['coverage'] = coverage_counts / item_num."""
    metrics = list(metrics)
    _check_names(metrics)
    cutoffs = [int(k) for k in cutoffs]
    ids, hi = _pred_ids(pred, item_num)
    needs_gt = any(ops.N.KPI_IDS[m] <= ops.N.KPI_IDS["popularity"] for m in metrics)
    users = gt = gt_max = None
    if needs_gt:
        gt, users, gt_max = _truths(gt_csr_or_test_ur, test_u)
        if users.size != ids.shape[0]:
            raise ValueError(f"test_u: {users.size} users for {ids.shape[0]} lists")
    if item_num is None:
        item_num = max(hi, gt_max or 0) + 1
    cat_np = n_cats = None
    if "diversity" in metrics:
        if i_categories is None:
            raise ValueError("'diversity' needs i_categories")
        cat_np, n_cats = pack_categories(i_categories)
        if cat_np.shape[0] < item_num:
            raise ValueError(f"i_categories: {cat_np.shape[0]} rows for item_num={item_num}")
    pop_np = None
    if "popularity" in metrics:
        if item_pop is None:
            raise ValueError("'popularity' needs item_pop")
        pop_np = np.ascontiguousarray(np.asarray(item_pop, dtype=np.float64).reshape(-1))
        if pop_np.size < item_num:
            raise ValueError(f"item_pop: {pop_np.size} entries for item_num={item_num}")

    dev = ids.device if isinstance(ids, torch.Tensor) and ids.is_cuda else _require_device()
    _require_device()
    pred_d = (ids if isinstance(ids, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ids))).to(dev)
    n, K = pred_d.shape
    if needs_gt:
        if isinstance(gt[0], torch.Tensor):
            indptr, gt_items = gt
            users_d = torch.from_numpy(users).to(dev)
            U = indptr.numel() - 1
            bad = (users_d < 0) | (users_d >= U)
            if not bool(bad.any()):
                bad = indptr[users_d + 1] == indptr[users_d]
            if bool(bad.any()):
                raise ValueError(f"user {int(users_d[bad][0])} of test_u has no ground truth in the CSR")
        else:
            indptr, gt_items = user_csr(gt, int(gt[0].max()) + 1, dev)
            users_d = torch.from_numpy(users).to(dev)
        if gt_items.numel() == 0:
            gt_items = gt_items.new_zeros(1)
    else:                                                               # coverage / diversity: no truths are read
        indptr = torch.zeros(2, dtype=torch.int64, device=dev)
        gt_items = torch.zeros(1, dtype=torch.int32, device=dev)
        users_d = torch.zeros(n, dtype=torch.int64, device=dev)
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev)                                   # noqa: E731
    disc = up(1 / np.log2(np.arange(2, K + 2))) if "ndcg" in metrics else None
    sqrt_tab = up(np.sqrt(np.arange(n_cats + 1))) if cat_np is not None else None
    names, pu, means, cover = ops.ranking_kpis(pred_d, indptr, gt_items, users_d, cutoffs, metrics, item_num, disc=disc,
                                               item_pop=up(pop_np), cat_bits=up(cat_np), n_cats=n_cats or 0,
                                               sqrt_tab=sqrt_tab, per_user=per_user)
    means_h = means.cpu().numpy()
    out = {"cutoffs": cutoffs, "means": {nm: means_h[s] for s, nm in enumerate(names)}, "per_user": None,
           "coverage_counts": None}
    if cover is not None:
        out["coverage_counts"] = cover.cpu().numpy()
        out["means"]["coverage"] = out["coverage_counts"] / item_num     # metrics.py:102
    if per_user:
        pu_h = pu.cpu().numpy() if pu is not None else None
        out["per_user"] = {nm: pu_h[s] for s, nm in enumerate(names)}
    return out


def _one(name, pred_ur, test_ur=None, test_u=None, **kw):
    K = pred_ur.shape[1]
    if K > MAX_K:
        raise ValueError(f"pred_ur: lists of {K} positions above {MAX_K}")
    return np.float64(ranking_kpis(pred_ur, test_ur, test_u, [K], [name], **kw)["means"][name][0])


def Coverage(pred_ur, item_num):
    """metrics.py:98-102"""
    return _one("coverage", pred_ur, item_num=item_num)


def Popularity(test_ur, pred_ur, test_u, item_pop):
    """metrics.py:104-122"""
    return _one("popularity", pred_ur, test_ur, test_u, item_pop=item_pop)


def Diversity(pred_ur, i_categories):
    """metrics.py:124-146"""
    return _one("diversity", pred_ur, i_categories=i_categories)


def Precision(test_ur, pred_ur, test_u):
    """metrics.py:148-158"""
    return _one("precision", pred_ur, test_ur, test_u)


def Recall(test_ur, pred_ur, test_u):
    """metrics.py:160-170"""
    return _one("recall", pred_ur, test_ur, test_u)


def MRR(test_ur, pred_ur, test_u):
    """metrics.py:172-186"""
    return _one("mrr", pred_ur, test_ur, test_u)


def MAP(test_ur, pred_ur, test_u):
    """metrics.py:188-202"""
    return _one("map", pred_ur, test_ur, test_u)


def NDCG(test_ur, pred_ur, test_u):
    """metrics.py:204-227"""
    return _one("ndcg", pred_ur, test_ur, test_u)


def HR(test_ur, pred_ur, test_u):
    """metrics.py:229-239"""
    return _one("hit", pred_ur, test_ur, test_u)


def AUC(test_ur, pred_ur, test_u):
    """metrics.py:241-261"""
    return _one("auc", pred_ur, test_ur, test_u)


def F1(test_ur, pred_ur, test_u):
    """metrics.py:263-278"""
    return _one("f1", pred_ur, test_ur, test_u)


class Metric(object):
    """metrics.py:59-96"""

    def __init__(self, config) -> None:
        self.metrics = config['metrics']
        self.item_num = config['item_num']
        self.item_pop = config['item_pop'] if ('coverage' in self.metrics or 'popularity' in self.metrics) else None
        self.i_categories = config['i_categories'] if 'diversity' in self.metrics else None

    def _kpis(self, test_ur, pred_ur, test_u, cutoffs):
        _check_names(self.metrics)
        return ranking_kpis(pred_ur, test_ur, test_u, cutoffs, list(dict.fromkeys(self.metrics)), item_num=self.item_num,
                            item_pop=self.item_pop if 'popularity' in self.metrics else None,
                            i_categories=self.i_categories)["means"]

    def run(self, test_ur, pred_ur, test_u):
        means = self._kpis(test_ur, pred_ur, test_u, [pred_ur.shape[1]])
        return [np.float64(means[mc][0]) for mc in self.metrics]


def calc_ranking_results(test_ur, pred_ur, test_u, config):
    """metrics.py:18-57: the DataFrame of every KPI of config['metrics'] at the cutoffs 1, 5, 10, 20, 30, 50 and
    config['topk'] (those above config['topk'] skipped), from ONE device call."""
    import pandas as pd
    logger = config['logger']
    path = config['res_path']
    if not os.path.exists(path):
        os.makedirs(path)

    metric = Metric(config)
    _check_names(metric.metrics)
    res = pd.DataFrame({
        'KPI@K': [metrics_name_config[kpi_name] for kpi_name in config['metrics']]
    })

    common_ks = [1, 5, 10, 20, 30, 50]
    if config['topk'] not in common_ks:
        common_ks.append(config['topk'])
    order = [topk for topk in common_ks if topk <= config['topk']]
    ks = sorted(order)
    if ks and ks[-1] > pred_ur.shape[1]:
        raise ValueError(f"config['topk']={config['topk']} above the {pred_ur.shape[1]} ranked positions of pred_ur")
    means = metric._kpis(test_ur, pred_ur[:, :ks[-1]], test_u, ks)
    for topk in order:
        kpis = [np.float64(means[mc][ks.index(topk)]) for mc in config['metrics']]
        if topk == 10:
            for kpi_name, kpi_res in zip(config['metrics'], kpis):
                kpi_name = metrics_name_config[kpi_name]
                logger.info(f'{kpi_name}@{topk}: {kpi_res:.4f}')

        res[topk] = np.array(kpis)

    return res


def position_kpis(out_indptr, positions, gt_len, eligible, cutoffs, metrics, per_user=False):
    """ranking_kpis from the exact rank positions of the held-out items (ops.full_rank_positions): every
    per-list KPI of `metrics` - 'precision', 'recall', 'hit', 'mrr', 'map', 'ndcg', 'f1', 'auc', with the reference's list
    definitions applied to the implied list of length K, and 'full_auc', the exact AUC over all eligible items - at
    every cutoff (strictly ascending, ANY K >= 1) in one device call.  gt_len: the truths of every request (None: the
    length of its row).  Where K exceeds a user's eligible items the implied list is that short: precision and auc
    use min(K, eligible).  'popularity', 'diversity' and 'coverage' need the lists and raise ValueError.  -> the dict
    of ranking_kpis ('coverage_counts' is None)."""
    metrics = list(dict.fromkeys(metrics))
    cutoffs = [int(k) for k in cutoffs]
    dev = positions.device
    if gt_len is not None:
        gt_len = torch.as_tensor(gt_len).to(device=dev, dtype=torch.int64).contiguous()
    eligible = torch.as_tensor(eligible).to(device=dev, dtype=torch.int32).contiguous()
    disc = cum = None
    if "ndcg" in metrics:                   # the discounts of every position a hit can have, as ranking_kpis builds them
        top = int(positions.max()) + 1 if positions.numel() else 0
        d_np = 1 / np.log2(np.arange(2, max(1, min(max(cutoffs, default=1), top)) + 2))
        disc, cum = torch.from_numpy(d_np).to(dev), torch.from_numpy(np.cumsum(d_np)).to(dev)
    names, pu, means = ops.position_kpis(out_indptr, positions.contiguous(), gt_len, eligible, cutoffs, metrics, disc=disc,
                                         disc_cum=cum, per_user=per_user)
    means_h = means.cpu().numpy()
    out = {"cutoffs": cutoffs, "means": {nm: means_h[s] for s, nm in enumerate(names)}, "per_user": None,
           "coverage_counts": None}
    if per_user:
        pu_h = pu.cpu().numpy()
        out["per_user"] = {nm: pu_h[s] for s, nm in enumerate(names)}
    return out


def calc_full_ranking_results(model, test_ur, train_ur, config):
    """calc_ranking_results under the full-ranking protocol, from ONE model.full_rank_positions call over the users of
    test_ur (every item outside the user's train_ur row is a candidate) and one KPI call: the same DataFrame - the
    columns 'KPI@K', 1, 5, 10, 20, 30, 50 and config['topk'], those above config['topk'] skipped - and the same @10 log
    lines.  config['topk'] has no upper bound here, and a user with fewer eligible items than a cutoff is not refused
    (position_kpis).  config['metrics'] may hold 'full_auc'."""
    import pandas as pd
    logger = config['logger']
    path = config['res_path']
    if not os.path.exists(path):
        os.makedirs(path)
    names = dict(metrics_name_config, full_auc='AUC (all items)')
    for mc in config['metrics']:
        if mc not in names:
            raise ValueError(f'Invalid metric name {mc}')
    users = np.asarray(list(test_ur.keys()), dtype=np.int64)
    for u in users.tolist():
        if len(test_ur[u]) == 0:
            raise ValueError(f"user {u} of test_u has no ground truth in test_ur")
    res = pd.DataFrame({'KPI@K': [names[kpi_name] for kpi_name in config['metrics']]})
    common_ks = [1, 5, 10, 20, 30, 50]
    if config['topk'] not in common_ks:
        common_ks.append(config['topk'])
    order = [topk for topk in common_ks if topk <= config['topk']]
    ks = sorted(order)
    out_indptr, pos, eligible = model.full_rank_positions(users, test_ur, exclude=train_ur, return_eligible=True)
    means = position_kpis(out_indptr, pos, None, eligible, ks, config['metrics'])["means"]
    for topk in order:
        kpis = [np.float64(means[mc][ks.index(topk)]) for mc in config['metrics']]
        if topk == 10:
            for kpi_name, kpi_res in zip(config['metrics'], kpis):
                logger.info(f'{names[kpi_name]}@{topk}: {kpi_res:.4f}')
        res[topk] = np.array(kpis)
    return res
