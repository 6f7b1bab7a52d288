"""Mirror of `daisy.utils.splitter` (splitter.py:4-185) on the HIP path: `TestSplitter`, `ValidationSplitter`,
`split_test`, `split_validation` with the reference's signatures, on any frame (the user column is encoded first).  The
per-user methods are one library call (`daisy_split_ids`, csrc/split.hip) instead of `groupby(uid).apply(<lambda>)`;
`tsbr` and `cv` are index arithmetic on the host.  Ids are int64 ndarrays of positions (the reference returns labels of a
`RangeIndex`: the same numbers; for ufo / utfo an object array, for rloo a Series - all only ever fed to `df.iloc`).
`split_validation` returns a `zip` of `(train_ids, val_ids)` per fold.

`seed` is `config['seed']` (2022 when absent), as in `build_candidates_set`; the functions take it as an extra keyword.

Deviations from the reference:
  * `utfo` takes each user's own last rows.  The reference returns the global range [first + split_len, last] of every
    user - the same rows whenever every user's rows are contiguous, duplicated foreign rows otherwise.
  * the random methods (`rsbr`, `ufo`, `rloo`) use the library's counter-based generator, keyed by (seed, fold, row),
    not `np.random` / `DataFrame.sample`: the same sizes and the same distribution, other draws.  `test_ids` come users
    ascending, then by key.
  * a `ufo` user with `round(len * size) == 0` contributes nothing (the reference's `explode` yields NaN there and
    `iloc` fails).
  * `cv` has scikit-learn's unshuffled `KFold` sizes (the first n % k folds get one row more); the reference's own call
    passes `random_state` with `shuffle=False`, which current scikit-learn refuses.
There is no CPU path for the per-user and random methods: without a HIP device they raise.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .loader import id_column, int64_column

DEFAULT_SEED = 2022
TEST_METHODS = ("rsbr", "tsbr", "tloo", "rloo", "ufo", "utfo")
VAL_METHODS = TEST_METHODS + ("cv",)


class TestSplitter(object):
    __test__ = False            # not a pytest class

    def __init__(self, config):
        self.test_method = config['test_method']
        self.test_size = config['test_size']
        self.uid = config['UID_NAME']
        self.tid = config['TID_NAME']
        self.seed = _config_seed(config)

    def split(self, df):
        return split_test(df, self.test_method, self.test_size, self.uid, self.tid, seed=self.seed)


class ValidationSplitter(object):
    def __init__(self, config):
        self.val_method = config['val_method']
        self.fold_num = config['fold_num']
        self.val_size = config['val_size']
        self.uid = config['UID_NAME']
        self.tid = config['TID_NAME']
        self.seed = _config_seed(config)

    def split(self, df):
        return split_validation(df, self.val_method, self.fold_num, self.val_size, self.uid, self.tid, seed=self.seed)


def _config_seed(config):
    try:
        seed = config['seed']
    except (KeyError, IndexError):
        seed = None
    return DEFAULT_SEED if seed is None else int(seed)


def _check_size(size):
    size = float(size)
    if not 0.0 < size < 1.0:
        raise ValueError(f"split size {size} outside (0, 1)")
    return size


def _device_split(df, method, size, uid, tid, seed, fold, device="cuda"):
    """one (train_ids, test_ids) of a method that needs the device"""
    n = len(df)
    sized = method in ("rsbr", "ufo", "utfo")
    if sized:
        size = _check_size(size)
    users = ts = None
    if method != "rsbr":
        users, _ = id_column(df[uid])
    if method == "tloo":
        ts = int64_column(df[tid], f"column {tid!r}")
    if not torch.cuda.is_available():
        raise RuntimeError(f"daisyrec_amd.split_test({method!r}) needs a HIP device (no CPU fallback)")
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    code, user_num = None, 0
    if users is not None:
        code, tokens = ops.prep_encode(torch.from_numpy(users).to(device))
        user_num = tokens.numel()
    tsd = None if ts is None else torch.from_numpy(ts).to(device)
    train, test = ops.split_ids(method, n, user_code=code, user_num=user_num, timestamp=tsd, size=size if sized else 0.5,
                                seed=seed, fold=fold, device=device)
    return train.cpu().numpy(), test.cpu().numpy()


def _tsbr(n, size):
    split_idx = int(np.ceil(n * (1 - _check_size(size))))           # splitter.py:71
    return np.arange(split_idx), np.arange(split_idx, n)


def split_test(df, test_method='rsbr', test_size=.2, uid='user', tid='timestamp', seed=DEFAULT_SEED):
    """splitter.py:29-91 -> (train_ids, test_ids), int64 positions"""
    if test_method not in TEST_METHODS:
        raise ValueError('Invalid data_split value, expect: rloo, rsbr, tloo, tsbr')
    if test_method == 'tsbr':
        return _tsbr(len(df), test_size)
    return _device_split(df, test_method, test_size, uid, tid, seed, 0)


def split_validation(train_set, val_method='rsbr', fold_num=1, val_size=.1, uid='user', tid='timestamp', seed=DEFAULT_SEED):
    """splitter.py:94-185 -> zip of (train_ids, val_ids) per fold.  Fold f of a random method draws from stream f + 1 of
    the seed (stream 0 is split_test's), so a validation fold never repeats the test draw."""
    if val_method not in VAL_METHODS:
        raise ValueError(f'Invalid val_method value {val_method!r}, expect one of: ' + ', '.join(VAL_METHODS))
    n = len(train_set)
    pairs = []
    if val_method == 'cv':
        fold_num = int(fold_num)
        if fold_num < 2 or fold_num > n:
            raise ValueError(f"cv needs 2 <= fold_num <= len(train_set) = {n}, got {fold_num}")
        sizes = np.full(fold_num, n // fold_num, dtype=np.int64)
        sizes[:n % fold_num] += 1
        stop = np.cumsum(sizes)
        ids = np.arange(n)
        for a, b in zip(stop - sizes, stop):
            pairs.append((np.concatenate([ids[:a], ids[b:]]), ids[a:b]))
    elif val_method == 'tsbr':
        pairs.append(_tsbr(n, val_size))
    elif val_method in ('tloo', 'utfo'):
        pairs.append(_device_split(train_set, val_method, val_size, uid, tid, seed, 0))
    else:
        for f in range(int(fold_num)):
            pairs.append(_device_split(train_set, val_method, val_size, uid, tid, seed, f + 1))
    return zip([p[0] for p in pairs], [p[1] for p in pairs])
