"""Loader boundary (reference: daisy/utils/dataset.py:5-27).

``BasicDataset`` / ``get_dataloader`` keep the reference's names and behaviour so
callers (run_examples/test.py:93-94) are unchanged; the native ``MF.fit`` never
iterates the DataLoader — it reads ``dataset.data`` (the int32 [N,3] triples) once,
moves it to HBM and replays the loader's index order on the device.

``DeviceTripleLoader`` is the throughput-mode loader: triples stay resident in HBM
and each epoch's order is a device-side Philox permutation.
"""
from __future__ import annotations

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from .. import ops


def get_dataloader(ds, batch_size, shuffle, num_workers=4):
    """dataset.py:5-7."""
    return DataLoader(ds, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers)


class BasicDataset(Dataset):
    """dataset.py:10-27: array-like <u, i, j> samples."""

    def __init__(self, samples):
        super().__init__()
        self.data = samples

    def __len__(self):
        return len(self.data)

    def __getitem__(self, index):
        row = self.data[index]
        return row[0], row[1], row[2]


class CandidatesDataset(Dataset):
    """dataset.py:29-38 (used by MF.rank's caller, test.py:118)."""

    def __init__(self, ucands):
        super().__init__()
        self.data = ucands

    def __len__(self):
        return len(self.data)

    def __getitem__(self, index):
        return torch.tensor(self.data[index][0]), torch.tensor(self.data[index][1])


class AEDataset(Dataset):
    """dataset.py:40-58: the distinct values of `train_set[yield_col]` in order of first appearance (what
    `Series.unique()` returns), one per sample.  The order comes from the device (ops.history_first_seen: the first frame
    position of every id, then a compaction in frame order); `.data` is the host int64 vector the reference holds -
    `VAECF.fit` reads it from there.  Ids that are not small non-negative integers go through their dense codes first
    (ops.prep_encode).  There is no CPU path."""

    def __init__(self, train_set, yield_col='user'):
        super().__init__()
        ids = np.asarray(train_set[yield_col].values)
        if ids.dtype.kind not in "iu":
            raise TypeError(f"AEDataset: column {yield_col!r} has dtype {ids.dtype}; integer ids expected")
        if not torch.cuda.is_available():
            raise RuntimeError("daisyrec_amd.AEDataset needs a HIP device (no CPU fallback)")
        n = ids.size
        if n == 0:
            self.data = np.zeros(0, dtype=np.int64)
            return
        lo, hi = int(ids.min()), int(ids.max())
        if lo >= 0 and hi < max(4 * n, 1 << 20):
            codes = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).cuda()
            first = ops.history_first_seen(codes, hi + 1, validate=False)
        else:           # raw ids: rank them first, order the ranks, read the ids back
            codes, tokens = ops.prep_encode(torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).cuda())
            first = tokens[ops.history_first_seen(codes, tokens.numel(), validate=False)]
        self.data = first.cpu().numpy().astype(np.int64, copy=False)

    def __len__(self):
        return len(self.data)

    def __getitem__(self, index):
        return self.data[index]


class DeviceTripleLoader:
    """HBM-resident triples + per-epoch device permutation (shuffle=True semantics:
    every epoch is a fresh uniform permutation; last batch partial)."""

    def __init__(self, triples, batch_size, shuffle=True, seed=2022, device="cuda"):
        t = torch.as_tensor(np.asarray(triples) if not isinstance(triples, torch.Tensor) else triples)
        self.triples = t.to(torch.int32).contiguous().to(device)
        self.batch_size = int(batch_size)
        self.shuffle = bool(shuffle)
        self.seed = int(seed)
        self.epoch = 0

    def __len__(self):
        return (self.triples.shape[0] + self.batch_size - 1) // self.batch_size

    def next_epoch_order(self):
        """int64 device permutation for the next epoch (None when not shuffling)."""
        e = self.epoch
        self.epoch += 1
        if not self.shuffle:
            return None
        return ops.randperm(self.triples.shape[0], self.seed, e, device=self.triples.device)
