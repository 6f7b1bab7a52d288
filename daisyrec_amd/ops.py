"""Tensor-level operators over the C ABI (``include/daisyrec_amd.h``).

PyTorch is plumbing here: it owns device memory and streams; every operator
hands raw device pointers + the current HIP stream to ``libdaisyrec_hip.so``.
Nothing in this module computes on the host or falls back to torch ops.
"""
from __future__ import annotations

import ctypes as C
import weakref

import torch

from . import _native as N
from ._native import check, lib

LOSS_IDS = {"BPR": N.LOSS_BPR, "HL": N.LOSS_HL, "TL": N.LOSS_TL, "CL": N.LOSS_CL, "SL": N.LOSS_SL}
POINTWISE_LOSSES = (N.LOSS_CL, N.LOSS_SL)
ITEM_MODES = {"atomic": N.ITEM_ATOMIC, "sorted": N.ITEM_SORTED, "chunked": N.ITEM_CHUNKED,
              "fused": N.ITEM_FUSED}
SMALL_BATCH_MAX = 256      # kSmallBatchMax (csrc/bpr_internal.h): fit_epoch_sgd runs such epochs in one persistent workgroup
SMALL_LDS_ROW_BYTES = 128 * 1024      # kSmallLdsRows (csrc/bpr_small.hip): a batch's user rows, float4-padded, must fit in it
ORDER_MODES = {"identity": N.ORDER_IDENTITY, "perm": N.ORDER_PERM, "feistel": N.ORDER_FEISTEL}


def loss_id(loss_type: str) -> int:
    key = str(loss_type).upper()
    if key not in LOSS_IDS:
        # MFRecommender.py:90-91 / AbstractRecommender.py:91
        raise NotImplementedError(f"Invalid loss type: {loss_type}")
    return LOSS_IDS[key]


def _ptr(t, dtype, name):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor is on {t.device}; the HIP path needs device memory "
                           "(there is no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rows(t, name):
    """(pointer, row pitch) of a 2-D float32 device tensor whose rows are contiguous: a whole matrix or a column
    slice of a wider one (NGCF's concat buffer)."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise TypeError(f"{name}: expected a 2-D torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor is on {t.device}; the HIP path needs device memory "
                           "(there is no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected dtype torch.float32, got {t.dtype}")
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError(f"{name}: rows must be contiguous")
    return C.c_void_p(t.data_ptr()), max(int(t.stride(0)), int(t.shape[1]))


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


class _Native:
    """Owner of one native handle (`_h`).  A subclass names the library's destroy function and, where there is one, its
    bytes function.  close() may be called twice, and after a constructor that failed before the handle was set; the
    object is not usable after it."""

    _destroy = None
    _bytes = None

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            check(type(self)._destroy(h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def nbytes(self):
        return int(type(self)._bytes(self._h))


class TrainIndex(_Native):
    """Owner of a native ``daisy_train_index``: the training triples in CSR order + their item entries
    sorted by item, built once per fit (BasicDataset's triple array is immutable, dataset.py:21).
    Raises ValueError when an id lies outside the tables (the reference: IndexError in nn.Embedding)."""

    _destroy = lib.daisy_train_index_destroy
    _bytes = lib.daisy_train_index_bytes

    def __init__(self, triples, user_num: int, item_num: int, user_base: int = 0, user_sorted=None, pointwise=False):
        """pointwise: rows are (user, item, label) (CL / SL, sampler.py:93-98): one item entry per row"""
        if user_sorted is None:
            user_sorted = triples_user_sorted(triples)
        self.triples = triples            # kept alive: a user-sorted array is indexed in place
        self.n = int(triples.shape[0])
        self.user_num, self.item_num = int(user_num), int(item_num)
        self._h = C.c_void_p()
        with torch.cuda.device(triples.device):
            check(lib.daisy_train_index_create(C.byref(self._h), _ptr(triples, torch.int32, "triples"), self.n,
                                               self.user_num, self.item_num, int(user_base),
                                               (N.PLAN_TRIPLES_USER_SORTED if user_sorted else 0)
                                               | (N.PLAN_POINTWISE if pointwise else 0), _stream()))

class EpochPlan(_Native):
    """Owner of a native ``daisy_epoch_plan``: one epoch laid out batch by batch in HBM
    (replaces a pass over DataLoader(BasicDataset(triples)), dataset.py:5-27)."""

    _destroy = lib.daisy_epoch_plan_destroy
    _bytes = lib.daisy_epoch_plan_bytes

    def __init__(self, max_triples: int, user_num: int, item_num: int, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("EpochPlan needs a HIP device (no CPU fallback)")
        self.max_triples = int(max_triples)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib.daisy_epoch_plan_create(C.byref(self._h), self.max_triples, int(user_num),
                                              int(item_num)))

    def build(self, triples, batch_size, order="identity", perm=None, seed=0, epoch=0, user_base=0,
              n_triples=None, user_sorted=False, pointwise=False, validate=None):
        """user_sorted=True promises that `triples` is sorted by user (use `triples_user_sorted`
        to check once): grouping by user then costs one radix pass instead of a full sort.
        validate: check the id ranges after the build (one host sync; ValueError like the reference's
        IndexError).  Default: the first build over a given triple array (and every explicit permutation)."""
        n = triples.shape[0] if n_triples is None else int(n_triples)
        mode = ORDER_MODES[order] if isinstance(order, str) else int(order)
        flags = (N.PLAN_TRIPLES_USER_SORTED if user_sorted else 0) | (N.PLAN_POINTWISE if pointwise else 0)
        check(lib.daisy_epoch_plan_build(self._h, _ptr(triples, torch.int32, "triples"), n,
                                         _ptr(perm, torch.int64, "perm"), mode, int(seed), int(epoch),
                                         int(batch_size), int(user_base), flags, _stream()))
        if validate is None:       # the same tensor object, unchanged since its last validated build, is not re-read
            ref = getattr(self, "_validated", None)
            same = ref is not None and ref[0]() is triples and ref[1:] == (n, int(user_base), triples._version)
            validate = (not same) or mode == N.ORDER_PERM
        if validate:
            check(lib.daisy_epoch_plan_validate(self._h, _stream()))
            self._validated = (weakref.ref(triples), n, int(user_base), triples._version)
        return self

    def build_indexed(self, index: "TrainIndex", batch_size, order="identity", perm=None, seed=0, epoch=0):
        """The partitioned layout (32 B per interaction, two one-digit partitions of the static index
        instead of two radix sorts); feeds the staged step (item_mode 'fused') only."""
        mode = ORDER_MODES[order] if isinstance(order, str) else int(order)
        check(lib.daisy_epoch_plan_build_indexed(self._h, index._h, _ptr(perm, torch.int64, "perm"), mode,
                                                 int(seed), int(epoch), int(batch_size), _stream()))
        return self

    def build_positions(self, index: "TrainIndex", positions, n_total, batch_size):
        """One rank's share of an epoch over n_total rows: `index` holds this rank's rows, positions[r] (int64,
        distinct, in [0, n_total)) the place of its row r in the epoch order; batch k = the held rows with position
        in [k*B, (k+1)*B) - the union over the ranks is batch k of the single-device epoch.  Batches differ in
        size (`batch_rows`); one host sync."""
        check(lib.daisy_epoch_plan_build_positions(self._h, index._h, _ptr(positions, torch.int64, "positions"),
                                                   int(n_total), int(batch_size), _stream()))
        return self

    def batch_rows(self, k):
        """rows of batch k held by this plan (host value)"""
        return int(lib.daisy_epoch_plan_batch_rows(self._h, int(k)))

    @property
    def num_batches(self):
        return int(lib.daisy_epoch_plan_num_batches(self._h))

    def read_batch(self, k, batch_size):
        """(u, i, j, ent_item, ent_s, ent_u) of batch k as device tensors (inspection / tests)."""
        dev = self.device
        u, i, j = (torch.empty(batch_size, dtype=torch.int32, device=dev) for _ in range(3))
        ei, es, eu = (torch.empty(2 * batch_size, dtype=torch.int32, device=dev) for _ in range(3))
        B = C.c_int64(0)
        check(lib.daisy_epoch_plan_read_batch(self._h, int(k), _ptr(u, torch.int32, "u"),
                                              _ptr(i, torch.int32, "i"), _ptr(j, torch.int32, "j"),
                                              _ptr(ei, torch.int32, "ent_item"), _ptr(es, torch.int32, "ent_s"),
                                              _ptr(eu, torch.int32, "ent_u"), C.byref(B), _stream()))
        b = B.value
        return u[:b], i[:b], j[:b], ei[:2 * b], es[:2 * b], eu[:2 * b]


def triples_user_sorted(triples) -> bool:
    """One-off check (plumbing, not the hot path) that a device triple array is in CSR order."""
    u = triples[:, 0]
    return bool((u[1:] >= u[:-1]).all().item()) if u.numel() > 1 else True


def feistel_positions(n, seed, epoch=0, device="cuda"):
    """pos[t] = position of triple t in the device shuffle of (seed, epoch)."""
    out = torch.empty(n, dtype=torch.int64, device=device)
    check(lib.daisy_feistel_positions(int(n), int(seed), int(epoch), _ptr(out, torch.int64, "out"),
                                      _stream()))
    return out


def feistel_positions_at(ids, n, seed, epoch=0):
    """pos[k] = position of triple ids[k] in the device shuffle of all n triples (a rank's rows of a multi-GPU fit)."""
    out = torch.empty(ids.shape[0], dtype=torch.int64, device=ids.device)
    if ids.numel() == 0:            # a rank without rows (the native entry rejects n_ids == 0)
        return out
    check(lib.daisy_feistel_positions_at(_ptr(ids, torch.int64, "ids"), ids.shape[0], int(n), int(seed), int(epoch),
                                         _ptr(out, torch.int64, "out"), _stream()))
    return out


class BprContext(_Native):
    """Owner of a native ``daisy_bpr_ctx`` (per-step scratch on one GPU)."""

    _destroy = lib.daisy_bpr_ctx_destroy
    _bytes = lib.daisy_bpr_ctx_scratch_bytes

    def __init__(self, max_batch: int, d: int, user_num: int, item_num: int, device="cuda"):
        self.max_batch, self.d, self.user_num, self.item_num = int(max_batch), int(d), int(user_num), int(item_num)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("BprContext needs a HIP device (no CPU fallback)")
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib.daisy_bpr_ctx_create(C.byref(self._h), self.max_batch, self.d, self.user_num,
                                           self.item_num))
        # caller-owned (so torch.distributed can all-reduce them)
        self.stats = torch.zeros(N.STATS_LEN, dtype=torch.float64, device=self.device)
        self.epoch_acc = torch.zeros(2, dtype=torch.float64, device=self.device)
        self.gQ = torch.zeros(self.item_num, self.d, dtype=torch.float32, device=self.device)
        self._p_key = None        # (data_ptr, torch version counter) of the P the row-norm cache describes
        self._bias = None

    def _sync_norm_cache(self, P):
        """The staged step keeps |P[u]|^2 per row inside the context.  The native side tracks every write
        that goes through it; torch-side in-place edits of P show up in the tensor's version counter."""
        key = (P.data_ptr(), P._version)
        if key != self._p_key:
            check(lib.daisy_bpr_ctx_invalidate_cache(self._h))
            self._p_key = key

    def invalidate_cache(self):
        check(lib.daisy_bpr_ctx_invalidate_cache(self._h))
        self._p_key = None

    def set_p_stream(self, mode="auto"):
        """staged step: user rows read / written past the caches ('auto': by table size - beyond 512 MB; True / False)"""
        m = -1 if mode in ("auto", None, -1) else (1 if mode else 0)
        check(lib.daisy_bpr_ctx_set_p_stream(self._h, m))

    # -- the staged step in phases (multi-GPU form) ------------------------------------------------
    def staged_prenorm(self, P):
        self._sync_norm_cache(P)
        check(lib.daisy_bpr_staged_prenorm(self._h, _ptr(P, torch.float32, "P"),
                                           _ptr(self.stats, torch.float64, "stats"), _stream()))

    def staged_user(self, P, Q, lr, reg_1, reg_2, loss_type=N.LOSS_BPR, gamma=1e-10):
        check(lib.daisy_bpr_staged_user(self._h, _ptr(P, torch.float32, "P"), _ptr(Q, torch.float32, "Q"),
                                        int(loss_type), float(gamma), float(lr), float(reg_1), float(reg_2),
                                        _ptr(self.stats, torch.float64, "stats"), _stream()))

    def staged_item(self, lr, reg_1, reg_2, Q=None, gQ=None, cnt=None, loss_type=N.LOSS_BPR):
        """Q given: SGD on the touched item rows in place.  gQ + cnt given instead: the data term of the
        item gradient and the per-item (n_pos, n_neg) for a reduce-scatter."""
        check(lib.daisy_bpr_staged_item(self._h, int(loss_type), _ptr(Q, torch.float32, "Q"),
                                        _ptr(gQ, torch.float32, "gQ"), _ptr(cnt, torch.float32, "cnt"),
                                        float(lr), float(reg_1), float(reg_2),
                                        _ptr(self.stats, torch.float64, "stats"), _stream()))

    def staged_adam_catchup_users(self, P, adam):
        """multi-GPU Adam: the rows of P the current batch references -> step adam.t - 1 (zero-gradient replays)"""
        self._sync_norm_cache(P)
        f = torch.float32
        check(lib.daisy_bpr_staged_adam_catchup_users(
            self._h, _ptr(P, f, "P"), _ptr(adam.mP, f, "mP"), _ptr(adam.vP, f, "vP"), _ptr(adam.lastP, torch.int32, "lastP"),
            _ptr(adam.table, f, "table"), adam.BETA1, adam.BETA2, adam.EPS, adam.t, _stream()))

    def staged_user_adam(self, P, Q, adam, reg_1, reg_2, loss_type=N.LOSS_BPR, gamma=1e-10):
        f = torch.float32
        check(lib.daisy_bpr_staged_user_adam(
            self._h, _ptr(P, f, "P"), _ptr(Q, f, "Q"), int(loss_type), float(gamma), adam.lr, float(reg_1), float(reg_2),
            _ptr(adam.mP, f, "mP"), _ptr(adam.vP, f, "vP"), _ptr(adam.lastP, torch.int32, "lastP"), adam.BETA1, adam.BETA2,
            adam.EPS, adam.t, _ptr(self.stats, torch.float64, "stats"), _stream()))

    def item_apply_counts_adam(self, Q_rows, g_rows, cnt_rows, m_rows, v_rows, adam, reg_1, reg_2):
        """The row owner's DENSE Adam step over its block of Q after the reduce-scatter of (g, cnt); clears g and cnt."""
        f = torch.float32
        check(lib.daisy_item_apply_counts_adam(
            _ptr(Q_rows, f, "Q"), _ptr(g_rows, f, "g"), _ptr(cnt_rows, f, "cnt"), _ptr(m_rows, f, "m"), _ptr(v_rows, f, "v"),
            Q_rows.shape[0], Q_rows.shape[1], adam.lr, float(reg_1), float(reg_2), adam.BETA1, adam.BETA2, adam.EPS, adam.t,
            _ptr(self.stats, torch.float64, "stats"), _stream()))

    def staged_item_slices(self, item_bounds):
        """Cut the item pass of the current batch at the given items (host ints, bounds[0] = 0, bounds[-1] >= item_num,
        at most 16 slices): `staged_item_slice(s, ...)` then reduces the entries of items [bounds[s], bounds[s+1])."""
        b = (C.c_int32 * len(item_bounds))(*[int(x) for x in item_bounds])
        check(lib.daisy_bpr_staged_item_slices(self._h, b, len(item_bounds) - 1, _stream()))

    def staged_item_slice(self, s, lr, reg_1, reg_2, gQ, cnt, loss_type=N.LOSS_BPR):
        check(lib.daisy_bpr_staged_item_slice(self._h, int(loss_type), _ptr(gQ, torch.float32, "gQ"),
                                              _ptr(cnt, torch.float32, "cnt"), int(s), float(lr), float(reg_1),
                                              float(reg_2), _ptr(self.stats, torch.float64, "stats"), _stream()))

    def item_apply_counts(self, Q_rows, g_rows, cnt_rows, lr, reg_1, reg_2):
        """The row owner's SGD step of a multi-GPU staged step: Q_rows -= lr*(g_rows + regulariser from the
        reduced entry counts and the finalized global norms); clears g_rows and cnt_rows."""
        item_apply_counts(Q_rows, g_rows, cnt_rows, lr, reg_1, reg_2, self.stats)

    scratch_bytes = _Native.nbytes

    def set_pointwise(self, flag):
        """Rows given to set_batch* are (user, item, label) - the CL / SL layout (sampler.py:93-98)."""
        check(lib.daisy_bpr_ctx_set_pointwise(self._h, int(bool(flag))))

    def set_bias(self, u_bias=None, i_bias=None, bias=None, g_u_bias=None, g_i_bias=None, g_bias=None):
        """Attach FM's bias parameters (FMRecommender.py:46-50); `set_bias()` detaches them.
        g_i_bias [I] is mandatory (zeroed scratch like gQ); g_u_bias [U] / g_bias [1] only for user_grad."""
        if u_bias is None:
            check(lib.daisy_bpr_ctx_set_bias(self._h, None, None, None, None, None, None))
            self._bias = None
            return
        f = torch.float32
        check(lib.daisy_bpr_ctx_set_bias(self._h, _ptr(u_bias.view(-1), f, "u_bias"), _ptr(i_bias.view(-1), f, "i_bias"),
                                         _ptr(bias.view(-1), f, "bias"), _ptr(g_u_bias, f, "g_u_bias"),
                                         _ptr(g_i_bias, f, "g_i_bias"), _ptr(g_bias, f, "g_bias")))
        self._bias = (u_bias, i_bias, bias, g_u_bias, g_i_bias, g_bias)     # keep the storage alive

    # -- batch -------------------------------------------------------------
    def set_batch_from_triples(self, triples, idx=None, start=0, B=None, user_base=0, validate=True):
        """validate: raise ValueError when an id lies outside the tables (one host sync; the reference raises
        IndexError in nn.Embedding).  Unvalidated out-of-range ids are treated as id 0, never dereferenced."""
        n = triples.shape[0]
        if B is None:
            B = idx.numel() if idx is not None else n - start
        check(lib.daisy_bpr_set_batch_from_triples(
            self._h, _ptr(triples, torch.int32, "triples"), n,
            _ptr(idx, torch.int64, "idx"), int(start), int(B), int(user_base), _stream()))
        if validate:
            check(lib.daisy_bpr_ctx_validate_batch(self._h, _stream()))

    def set_batch(self, u, i, j, validate=True):
        check(lib.daisy_bpr_set_batch(self._h, _ptr(u, torch.int32, "u"), _ptr(i, torch.int32, "i"),
                                      _ptr(j, torch.int32, "j"), u.numel(), _stream()))
        if validate:
            check(lib.daisy_bpr_ctx_validate_batch(self._h, _stream()))

    def set_batch_from_plan(self, plan, k):
        check(lib.daisy_bpr_set_batch_from_plan(self._h, plan._h, int(k), _stream()))

    # -- phases --------------------------------------------------------------
    def forward(self, P, Q, loss_type=N.LOSS_BPR, gamma=1e-10):
        check(lib.daisy_bpr_forward(self._h, _ptr(P, torch.float32, "P"), _ptr(Q, torch.float32, "Q"),
                                    int(loss_type), float(gamma),
                                    _ptr(self.stats, torch.float64, "stats"), _stream()))

    def finalize(self, reg_1, reg_2, step_loss=None, accumulate=True):
        check(lib.daisy_bpr_finalize(self._h, _ptr(self.stats, torch.float64, "stats"), float(reg_1),
                                     float(reg_2),
                                     _ptr(self.epoch_acc, torch.float64, "epoch_acc") if accumulate else None,
                                     _ptr(step_loss, torch.float64, "step_loss"), _stream()))

    def item_grad(self, P, Q, reg_1, reg_2, item_mode=N.ITEM_CHUNKED, gQ=None):
        gQ = self.gQ if gQ is None else gQ
        check(lib.daisy_bpr_item_grad(self._h, _ptr(P, torch.float32, "P"), _ptr(Q, torch.float32, "Q"),
                                      _ptr(self.stats, torch.float64, "stats"), float(reg_1),
                                      float(reg_2), _ptr(gQ, torch.float32, "gQ"), int(item_mode),
                                      _stream()))

    def item_grad_data(self, P, Q, item_mode=N.ITEM_CHUNKED, gQ=None):
        gQ = self.gQ if gQ is None else gQ
        check(lib.daisy_bpr_item_grad_data(self._h, _ptr(P, torch.float32, "P"), _ptr(Q, torch.float32, "Q"),
                                           _ptr(self.stats, torch.float64, "stats"),
                                           _ptr(gQ, torch.float32, "gQ"), int(item_mode), _stream()))

    def item_grad_reg(self, Q, reg_1, reg_2, gQ=None):
        gQ = self.gQ if gQ is None else gQ
        check(lib.daisy_bpr_item_grad_reg(self._h, _ptr(Q, torch.float32, "Q"),
                                          _ptr(self.stats, torch.float64, "stats"), float(reg_1),
                                          float(reg_2), _ptr(gQ, torch.float32, "gQ"), _stream()))

    def user_sgd(self, P, Q, lr, reg_1, reg_2):
        check(lib.daisy_bpr_user_sgd(self._h, _ptr(P, torch.float32, "P"), _ptr(Q, torch.float32, "Q"),
                                     _ptr(self.stats, torch.float64, "stats"), float(lr), float(reg_1),
                                     float(reg_2), _stream()))

    def user_grad(self, P, Q, reg_1, reg_2, gP):
        check(lib.daisy_bpr_user_grad(self._h, _ptr(P, torch.float32, "P"), _ptr(Q, torch.float32, "Q"),
                                      _ptr(self.stats, torch.float64, "stats"), float(reg_1),
                                      float(reg_2), _ptr(gP, torch.float32, "gP"), _stream()))

    def item_sgd_apply(self, Q, lr, dense=False, gQ=None):
        gQ = self.gQ if gQ is None else gQ
        check(lib.daisy_bpr_item_sgd_apply(self._h, _ptr(Q, torch.float32, "Q"),
                                           _ptr(gQ, torch.float32, "gQ"), float(lr), int(dense),
                                           _stream()))

    def sgd_step(self, P, Q, lr, reg_1, reg_2, loss_type=N.LOSS_BPR, gamma=1e-10,
                 item_mode=N.ITEM_CHUNKED, step_loss=None, accumulate=True):
        if item_mode == N.ITEM_FUSED:
            self._sync_norm_cache(P)
        check(lib.daisy_bpr_sgd_step(
            self._h, _ptr(P, torch.float32, "P"), _ptr(Q, torch.float32, "Q"), int(loss_type),
            float(gamma), float(lr), float(reg_1), float(reg_2), _ptr(self.gQ, torch.float32, "gQ"),
            _ptr(self.stats, torch.float64, "stats"),
            _ptr(self.epoch_acc, torch.float64, "epoch_acc") if accumulate else None,
            _ptr(step_loss, torch.float64, "step_loss"), int(item_mode), _stream()))

    def fit_epoch_sgd(self, plan, P, Q, lr, reg_1, reg_2, loss_type=N.LOSS_BPR, gamma=1e-10,
                      item_mode=N.ITEM_CHUNKED, step_losses=None):
        """Every batch of a built plan (one epoch), enqueued natively."""
        if item_mode == N.ITEM_FUSED:
            self._sync_norm_cache(P)
        check(lib.daisy_bpr_fit_epoch_sgd(
            self._h, plan._h, _ptr(P, torch.float32, "P"), _ptr(Q, torch.float32, "Q"),
            int(loss_type), float(gamma), float(lr), float(reg_1), float(reg_2),
            _ptr(self.gQ, torch.float32, "gQ"), _ptr(self.stats, torch.float64, "stats"),
            _ptr(self.epoch_acc, torch.float64, "epoch_acc"),
            _ptr(step_losses, torch.float64, "step_losses"), int(item_mode), _stream()))


def fit_epoch_sgd_many(trials, step_losses=None):
    """One SGD epoch of many independent small-batch models in one native call (daisy_bpr_fit_epoch_sgd_many): one
    workgroup per model, one launch per kernel shape.  `trials`: a list of (ctx, plan, P, Q, lr, reg_1, reg_2, loss_type,
    gamma), each what `ctx.fit_epoch_sgd(plan, P, Q, ...)` takes; every context's `epoch_acc` and `stats` are written as
    that call writes them, with the same bits.  step_losses: None, or one float64 tensor (or None) per trial with room
    for its plan's batches.  Two trials may share a plan, but not P, Q or a context; ValueError names the trial."""
    trials = list(trials)
    count = len(trials)
    if step_losses is None:
        step_losses = [None] * count
    if len(step_losses) != count:
        raise ValueError(f"step_losses: {len(step_losses)} entries for {count} trials")
    if count == 0:
        check(lib.daisy_bpr_fit_epoch_sgd_many(None, 0, None, 0, _stream()))
        return
    recs = (N.SmallTrial * count)()
    seen = {}
    for t, (trial, sl) in enumerate(zip(trials, step_losses)):
        ctx, plan, P, Q, lr, reg_1, reg_2, loss_type, gamma = trial
        if id(ctx) in seen:
            raise ValueError(f"fit_epoch_sgd_many: trial {t} shares its context (stats, epoch_acc) with trial {seen[id(ctx)]}")
        seen[id(ctx)] = t
        for W, rows, name in ((P, ctx.user_num, "P"), (Q, ctx.item_num, "Q")):
            if not isinstance(W, torch.Tensor) or tuple(W.shape) != (rows, ctx.d):
                raise ValueError(f"fit_epoch_sgd_many: trial {t}: {name} is not the [{rows}, {ctx.d}] table of its context")
        if sl is not None and sl.numel() < plan.num_batches:
            raise ValueError(f"fit_epoch_sgd_many: trial {t}: step_losses holds {sl.numel()} of {plan.num_batches} steps")
        r = recs[t]
        r.ctx, r.plan = ctx._h, plan._h
        r.P, r.Q = _ptr(P, torch.float32, "P"), _ptr(Q, torch.float32, "Q")
        r.loss_type, r.gamma, r.lr, r.reg_1, r.reg_2 = int(loss_type), float(gamma), float(lr), float(reg_1), float(reg_2)
        r.stats, r.epoch_acc = _ptr(ctx.stats, torch.float64, "stats"), _ptr(ctx.epoch_acc, torch.float64, "epoch_acc")
        r.step_losses = _ptr(sl, torch.float64, "step_losses")
    ctx0 = trials[0][0]
    with torch.cuda.device(ctx0.device):
        ws = _ws(count * N.SMALL_TRIAL_WS_BYTES, ctx0.device)
        check(lib.daisy_bpr_fit_epoch_sgd_many(recs, count, C.c_void_p(ws.data_ptr()), ws.numel(), _stream()))
    ctx0._many_ws = ws        # the kernels read it after this call returns: alive until the caller's next sync at least
    for trial in trials:
        trial[0]._p_key = None        # (the tables changed behind the row-norm cache, which the native side has dropped)


def item_apply_counts(Q, g, cnt, lr, reg_1, reg_2, stats):
    """Row owner's SGD step from reduced (g, cnt) (multi-GPU staged step); clears g and cnt."""
    check(lib.daisy_item_apply_counts(_ptr(Q, torch.float32, "Q"), _ptr(g, torch.float32, "g"),
                                      _ptr(cnt, torch.float32, "cnt"), Q.shape[0], Q.shape[1], float(lr),
                                      float(reg_1), float(reg_2), _ptr(stats, torch.float64, "stats"), _stream()))


def adam_dense(W, g, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-8):
    check(lib.daisy_adam_dense(_ptr(W, torch.float32, "W"), _ptr(g, torch.float32, "g"),
                               _ptr(m, torch.float32, "m"), _ptr(v, torch.float32, "v"), W.numel(),
                               float(lr), float(beta1), float(beta2), float(eps), int(step), _stream()))


def adagrad_dense(W, g, state_sum, lr, eps=1e-10):
    check(lib.daisy_adagrad_dense(_ptr(W, torch.float32, "W"), _ptr(g, torch.float32, "g"),
                                  _ptr(state_sum, torch.float32, "state_sum"), W.numel(), float(lr), float(eps), _stream()))


def rmsprop_dense(W, g, square_avg, lr, alpha=0.99, eps=1e-8):
    check(lib.daisy_rmsprop_dense(_ptr(W, torch.float32, "W"), _ptr(g, torch.float32, "g"),
                                  _ptr(square_avg, torch.float32, "square_avg"), W.numel(), float(lr), float(alpha),
                                  float(eps), _stream()))


class DenseOptimizer:
    """The dense torch optimisers of AbstractRecommender._build_optimizer (:48-67) on the native kernels, one
    state per parameter tensor: 'sgd', 'adam', 'adagrad', 'rmsprop' (torch defaults).  step() consumes and clears g."""

    KINDS = ("sgd", "adam", "adagrad", "rmsprop")

    def __init__(self, kind: str, lr: float):
        if kind not in self.KINDS:
            raise ValueError(f"DenseOptimizer: unknown kind {kind!r}")
        self.kind, self.lr, self.t, self._state = kind, float(lr), 0, {}

    def next_step(self):
        """Advance the (shared) step count: once per optimizer.step() of the reference."""
        self.t += 1

    def state_for(self, W):
        """The optimiser's state tensors of the flat parameter vector W (created zero at first use): () for SGD."""
        if self.kind == "sgd":
            return ()
        st = self._state.get(W.data_ptr())
        if st is None:
            st = self._state[W.data_ptr()] = tuple(torch.zeros_like(W) for _ in range(2 if self.kind == "adam" else 1))
        return st

    def native_args(self, W, g=None):
        """The optimiser as the library's fit_epoch entries take it: (kind index, lr, [W, g,] state0 or NULL, state1 or
        NULL) for the flat vectors W / g (g=None: an entry that takes W and g elsewhere in its signature)."""
        f = torch.float32
        st = self.state_for(W)
        vectors = (_ptr(W, f, "W"), _ptr(g, f, "g")) if g is not None else ()
        return (self.KINDS.index(self.kind), self.lr) + vectors + tuple(
            _ptr(st[k], f, f"state{k}") if len(st) > k else None for k in range(2))

    def step(self, W, g):
        W, g = W.view(-1), g.view(-1)
        if self.kind == "sgd":
            return sgd_dense(W, g, self.lr)
        st = self.state_for(W)
        if self.kind == "adam":
            adam_dense(W, g, st[0], st[1], self.lr, max(self.t, 1))
        elif self.kind == "adagrad":
            adagrad_dense(W, g, st[0], self.lr)
        else:
            rmsprop_dense(W, g, st[0], self.lr)


class LazyAdam:
    """torch.optim.Adam (defaults) on the two MF tables with traffic proportional to the rows a step touches, and the
    same bits as the dense form: rows without a gradient are replayed in registers when next needed
    (csrc/adam_lazy.hip: k_adam_batch_rows / k_adam_flush).  Usage per step: `catchup(ctx)` before the forward
    pass, `step(ctx, gP, gQ)` after the gradients; `flush()` before anything else reads the tables."""

    BETA1, BETA2, EPS = 0.9, 0.999, 1e-8

    def __init__(self, P, Q, lr, max_steps):
        self.P, self.Q, self.lr, self.t = P, Q, float(lr), 0
        self.m = [torch.zeros_like(P), torch.zeros_like(Q)]
        self.v = [torch.zeros_like(P), torch.zeros_like(Q)]
        self.last = [torch.zeros(P.shape[0], dtype=torch.int32, device=P.device),
                     torch.zeros(Q.shape[0], dtype=torch.int32, device=Q.device)]
        self._table_steps = 0
        self._table = None
        self._grow(max(int(max_steps), 1))

    def _grow(self, n_steps):
        host = (C.c_float * (2 * (n_steps + 1)))()
        check(lib.daisy_adam_lazy_table(self.lr, self.BETA1, self.BETA2, n_steps, host))
        self._table = torch.frombuffer(host, dtype=torch.float32).clone().to(self.P.device)
        self._table_steps = n_steps

    def catchup(self, ctx):
        self.t += 1
        if self.t > self._table_steps:
            self._grow(2 * self.t)
        self._ctx = ctx            # (flush() rewrites rows of P behind this context's row-norm cache)
        ctx._p_key = None          # the native side drops the cache; so does the wrapper's notion of it
        f = torch.float32
        check(lib.daisy_adam_lazy_catchup(
            ctx._h, _ptr(self.P, f, "P"), _ptr(self.m[0], f, "mP"), _ptr(self.v[0], f, "vP"),
            _ptr(self.last[0], torch.int32, "lastP"), _ptr(self.Q, f, "Q"), _ptr(self.m[1], f, "mQ"),
            _ptr(self.v[1], f, "vQ"), _ptr(self.last[1], torch.int32, "lastQ"), _ptr(self._table, f, "table"),
            self.BETA1, self.BETA2, self.EPS, self.t, _stream()))

    def step(self, ctx, gP, gQ):
        self._ctx = ctx
        ctx._p_key = None
        f = torch.float32
        check(lib.daisy_adam_lazy_step(
            ctx._h, _ptr(self.P, f, "P"), _ptr(gP, f, "gP"), _ptr(self.m[0], f, "mP"), _ptr(self.v[0], f, "vP"),
            _ptr(self.last[0], torch.int32, "lastP"), _ptr(self.Q, f, "Q"), _ptr(gQ, f, "gQ"), _ptr(self.m[1], f, "mQ"),
            _ptr(self.v[1], f, "vQ"), _ptr(self.last[1], torch.int32, "lastQ"), _ptr(self._table, f, "table"),
            self.BETA1, self.BETA2, self.EPS, self.t, _stream()))

    def staged_step(self, ctx, reg_1, reg_2, loss_type=N.LOSS_BPR, gamma=1e-10, step_loss=None, accumulate=True):
        """One Adam step on the current batch through the staged kernels (forward fused into the user update, item rows
        committed by their segment owner): catch-up of the rows the batch references, then step t on the rows that
        have a gradient.  FM contexts: the bias gradients land in the context's g_u_bias / g_i_bias and
        stats[ST_SUM_COEF] (bias_) for the caller's dense optimiser."""
        self.t += 1
        if self.t > self._table_steps:
            self._grow(2 * self.t)
        ctx._sync_norm_cache(self.P)
        self._ctx = ctx
        f = torch.float32
        check(lib.daisy_bpr_staged_adam_step(
            ctx._h, _ptr(self.P, f, "P"), _ptr(self.Q, f, "Q"), int(loss_type), float(gamma), self.lr, float(reg_1),
            float(reg_2), _ptr(self.m[0], f, "mP"), _ptr(self.v[0], f, "vP"), _ptr(self.last[0], torch.int32, "lastP"),
            _ptr(self.m[1], f, "mQ"), _ptr(self.v[1], f, "vQ"), _ptr(self.last[1], torch.int32, "lastQ"),
            _ptr(self._table, f, "table"), self.BETA1, self.BETA2, self.EPS, self.t,
            _ptr(ctx.stats, torch.float64, "stats"),
            _ptr(ctx.epoch_acc, torch.float64, "epoch_acc") if accumulate else None,
            _ptr(step_loss, torch.float64, "step_loss"), _stream()))

    @staticmethod
    def small_epoch_supported(ctx, plan, loss_type=N.LOSS_BPR) -> bool:
        """True when `fit_epoch` runs this (sorted-layout) plan's epochs inside one persistent workgroup
        (daisy_bpr_small_epoch_supported: B <= 256, pairwise loss, no FM biases, rows that fit the LDS)"""
        return bool(lib.daisy_bpr_small_epoch_supported(ctx._h, plan._h, int(loss_type)) & 1)

    @staticmethod
    def small_epoch_pays(ctx, plan, loss_type=N.LOSS_BPR) -> bool:
        """... and the Adam form is expected to be faster than the chain of launches (small tables: the rows a step references
        sat out a few steps; measured 35 against 48 us per step at ml-100k shapes, but 750 against 250 at 1 M x 100 K tables)"""
        return lib.daisy_bpr_small_epoch_supported(ctx._h, plan._h, int(loss_type)) == 3

    def fit_epoch(self, ctx, plan, reg_1, reg_2, loss_type=N.LOSS_BPR, gamma=1e-10, flush=True, step_losses=None):
        """Every batch of a built plan through the staged Adam step, enqueued by ONE native call (daisy_bpr_fit_epoch_adam:
        the loop of AbstractRecommender.py:118-128 without a host round trip per batch), then - flush - the rows no batch
        referenced brought up to the epoch's last step.  MF contexts only (FM's biases step between two steps)."""
        nb = plan.num_batches
        if self.t + nb > self._table_steps:
            self._grow(2 * (self.t + nb))
        ctx._sync_norm_cache(self.P)
        self._ctx = ctx
        f = torch.float32
        check(lib.daisy_bpr_fit_epoch_adam(
            ctx._h, plan._h, _ptr(self.P, f, "P"), _ptr(self.Q, f, "Q"), int(loss_type), float(gamma), self.lr,
            float(reg_1), float(reg_2), _ptr(self.m[0], f, "mP"), _ptr(self.v[0], f, "vP"),
            _ptr(self.last[0], torch.int32, "lastP"), _ptr(self.m[1], f, "mQ"), _ptr(self.v[1], f, "vQ"),
            _ptr(self.last[1], torch.int32, "lastQ"), _ptr(self._table, f, "table"), self._table_steps, self.BETA1,
            self.BETA2, self.EPS, self.t + 1, 1 if flush else 0, _ptr(ctx.stats, torch.float64, "stats"),
            _ptr(ctx.epoch_acc, torch.float64, "epoch_acc"), _ptr(step_losses, torch.float64, "step_losses"), _stream()))
        self.t += nb

    def flush(self):
        f = torch.float32
        for W, m, v, last in ((self.P, self.m[0], self.v[0], self.last[0]), (self.Q, self.m[1], self.v[1], self.last[1])):
            check(lib.daisy_adam_lazy_flush(_ptr(W, f, "W"), _ptr(m, f, "m"), _ptr(v, f, "v"),
                                            _ptr(last, torch.int32, "last"), W.shape[0], W.shape[1],
                                            _ptr(self._table, f, "table"), self.BETA1, self.BETA2, self.EPS, self.t,
                                            _stream()))
        ctx = getattr(self, "_ctx", None)              # the flush rewrote rows of P behind the staged step's row-norm cache
        if ctx is not None and getattr(ctx, "_h", None) is not None and ctx._h.value:
            ctx.invalidate_cache()
        else:                                          # (a context that was closed in the meantime has no cache to drop)
            self._ctx = None


class ShardedAdam:
    """torch.optim.Adam for the user-sharded step (sharding.UserShardedBprTrainer): the rank's rows of P in the lazy form
    (moments + stamps per local user; catch-up of a batch's rows before its forward, flush at the end), the rank's OWN
    block(s) of Q densely (every owned row steps in every step, like torch).  Same expressions as daisy_adam_dense."""

    BETA1, BETA2, EPS = 0.9, 0.999, 1e-8

    def __init__(self, P_local, owned_q_rows, d, lr, max_steps):
        dev = P_local.device
        self.P, self.lr, self.t = P_local, float(lr), 0
        self.mP, self.vP = torch.zeros_like(P_local), torch.zeros_like(P_local)
        self.lastP = torch.zeros(P_local.shape[0], dtype=torch.int32, device=dev)
        self.mQ = torch.zeros(owned_q_rows, d, dtype=torch.float32, device=dev)
        self.vQ = torch.zeros(owned_q_rows, d, dtype=torch.float32, device=dev)
        self._steps = 0
        self.table = None
        self._grow(max(int(max_steps), 1))

    def _grow(self, n_steps):
        host = (C.c_float * (2 * (n_steps + 1)))()
        check(lib.daisy_adam_lazy_table(self.lr, self.BETA1, self.BETA2, n_steps, host))
        self.table = torch.frombuffer(host, dtype=torch.float32).clone().to(self.P.device)
        self._steps = n_steps

    def next_step(self):
        self.t += 1
        if self.t > self._steps:
            self._grow(2 * self.t)

    def flush(self, ctx=None):
        """every local row of P up to the current step"""
        if self.t == 0 or self.P.shape[0] == 0:
            return
        f = torch.float32
        check(lib.daisy_adam_lazy_flush(_ptr(self.P, f, "W"), _ptr(self.mP, f, "m"), _ptr(self.vP, f, "v"),
                                        _ptr(self.lastP, torch.int32, "last"), self.P.shape[0], self.P.shape[1],
                                        _ptr(self.table, f, "table"), self.BETA1, self.BETA2, self.EPS, self.t, _stream()))
        if ctx is not None:
            ctx.invalidate_cache()


def _bias_ptrs(biases):
    if biases is None:
        return None, None, None
    bu, bi, b0 = biases
    f = torch.float32
    return _ptr(bu.view(-1), f, "u_bias"), _ptr(bi.view(-1), f, "i_bias"), _ptr(b0.view(-1), f, "bias")


def mf_predict(P, Q, u, i, biases=None):
    """MF.forward (MFRecommender.py:63-68); biases=(u_bias, i_bias, bias_): FM.forward (FMRecommender.py:61-68)."""
    u = u.to(torch.int64).contiguous()
    i = i.to(torch.int64).contiguous()
    out = torch.empty(u.numel(), dtype=torch.float32, device=P.device)
    if u.numel() == 0:
        return out
    bu, bi, b0 = _bias_ptrs(biases)
    check(lib.daisy_fm_predict(_ptr(P, torch.float32, "P"), _ptr(Q, torch.float32, "Q"), bu, bi, b0, P.shape[1],
                               _ptr(u, torch.int64, "u"), _ptr(i, torch.int64, "i"), u.numel(),
                               _ptr(out, torch.float32, "out"), _stream()))
    return out.view(u.shape)


def mf_rank_topk(P, Q, us, cands, topk, return_scores=False, biases=None):
    """One batch of MF.rank (MFRecommender.py:109-121) -> int64 [B, topk]; biases: FM.rank
    (FMRecommender.py:105-123)."""
    us = us.to(torch.int64).contiguous()
    cands = cands.to(torch.int64).contiguous()
    B, Cn = cands.shape
    topk = min(int(topk), int(Cn))          # rank_list[:, :topk] truncates (MFRecommender.py:119)
    out = torch.empty(B, topk, dtype=torch.int64, device=P.device)
    scores = torch.empty(B, Cn, dtype=torch.float32, device=P.device) if return_scores else None
    nbytes = lib.daisy_mf_rank_workspace_bytes(B, Cn)
    ws = _ws(nbytes, P.device)
    bu, bi, b0 = _bias_ptrs(biases)
    check(lib.daisy_fm_rank_topk(_ptr(P, torch.float32, "P"), _ptr(Q, torch.float32, "Q"), bu, bi, b0, P.shape[1],
                                 _ptr(us, torch.int64, "us"), _ptr(cands, torch.int64, "cands"), B, Cn,
                                 int(topk), _ptr(out, torch.int64, "out"),
                                 _ptr(scores, torch.float32, "scores"), _ptr(ws, torch.uint8, "ws"),
                                 ws.numel(), _stream()))
    return (out, scores) if return_scores else out


def mf_full_rank(P, Q, u, topk, biases=None):
    """MF.full_rank (MFRecommender.py:126-133) -> int64 [topk]; biases: FM.full_rank (FMRecommender.py:125-133)."""
    I = Q.shape[0]
    topk = min(int(topk), int(I))           # argsort(...)[:topk] truncates (MFRecommender.py:131)
    out = torch.empty(topk, dtype=torch.int64, device=P.device)
    ws = _ws(lib.daisy_mf_full_rank_workspace_bytes(I), P.device)
    bu, bi, b0 = _bias_ptrs(biases)
    check(lib.daisy_fm_full_rank(_ptr(P, torch.float32, "P"), _ptr(Q, torch.float32, "Q"), bu, bi, b0, P.shape[1], I,
                                 int(u), int(topk), _ptr(out, torch.int64, "out"),
                                 _ptr(ws, torch.uint8, "ws"), ws.numel(), _stream()))
    return out


FULL_RANK_TOPK_CAP = 128      # kFrTopkCap (csrc/rank_full.hip): the candidate buffers of a user tile live in LDS


def _check_exclusion(indptr, items, user_num):
    """ValueError unless (indptr, items) is a CSR over user_num rows whose rows are ascending (duplicates allowed):
    what build_user_csr returns.  Two device reductions, each read back once."""
    if indptr.dim() != 1 or items.dim() != 1 or indptr.numel() != user_num + 1:
        raise ValueError(f"exclude: indptr has {indptr.numel()} entries, the user table has {user_num} rows "
                         f"(expected {user_num + 1})")
    nnz = items.numel()
    steps_ok = bool(((indptr[1:] >= indptr[:-1]).all() & (indptr[0] == 0) & (indptr[-1] == nnz)).item())
    if not steps_ok:
        raise ValueError(f"exclude: indptr must rise from 0 to len(items) = {nnz}")
    if nnz > 1:
        inside = torch.ones(nnz + 1, dtype=torch.bool, device=items.device)
        inside[indptr] = False                                  # position p starts a row: nothing to compare with
        if bool(((items[1:] < items[:-1]) & inside[1:nnz]).any().item()):
            raise ValueError("exclude: the items of a row must be ascending (utils.user_csr / ops.build_user_csr sort them)")


def full_rank_users(P, Q, users, topk, exclude=None, biases=None, return_scores=False, item_slices=0, validate=True):
    """Full ranking of many users in two launches (csrc/rank_full.hip): int64 [n, min(topk, I)] device
    ids of the best items of ALL I by <P[u], Q[i]> (+ FM's biases), best first, equal scores by ascending id, without
    the items of the user's row of `exclude` = (indptr int64 [U + 1], items int32 ascending per row), the device CSR of
    build_user_csr.  A user with fewer eligible items than topk gets -1 (score -inf) in the remaining positions.
    return_scores: (ids, float32 scores).  topk above FULL_RANK_TOPK_CAP raises ValueError.  validate: IndexError for a
    user id outside [0, U), ValueError for an exclusion that is not such a CSR (one read-back each); False skips both -
    the kernel then trusts the ids and indptr, and only ever compares row contents."""
    U, I = int(P.shape[0]), int(Q.shape[0])
    if P.dim() != 2 or Q.dim() != 2 or P.shape[1] != Q.shape[1]:
        raise ValueError(f"full_rank_users: P {tuple(P.shape)} and Q {tuple(Q.shape)} need the same column count")
    users = torch.as_tensor(users).to(device=P.device, dtype=torch.int64).reshape(-1).contiguous()
    n = users.numel()
    topk = min(int(topk), I)                # as mf_full_rank: argsort(...)[:topk] truncates
    ids = torch.empty(n, topk, dtype=torch.int64, device=P.device)
    scores = torch.empty(n, topk, dtype=torch.float32, device=P.device) if return_scores else None
    indptr = items = None
    if exclude is not None:
        indptr, items = exclude
        if items.numel() == 0:              # (an empty tensor has no pointer to hand over)
            items = torch.zeros(1, dtype=torch.int32, device=P.device)
    if n and validate:
        lo, hi = (int(x) for x in torch.stack([users.min(), users.max()]).tolist())
        if lo < 0 or hi >= U:
            raise IndexError(f"index {hi if hi >= U else lo} is out of bounds for the user table with {U} rows")
        if exclude is not None:
            _check_exclusion(indptr, exclude[1], U)
    if n:
        ws = _ws(lib.daisy_full_rank_users_workspace_bytes(n, I, topk, int(item_slices)), P.device)
        bu, bi, b0 = _bias_ptrs(biases)
        check(lib.daisy_full_rank_users(_ptr(P, torch.float32, "P"), _ptr(Q, torch.float32, "Q"), bu, bi, b0, P.shape[1], I,
                                        _ptr(users, torch.int64, "users"), n, _ptr(indptr, torch.int64, "exclude indptr"),
                                        _ptr(items, torch.int32, "exclude items"), topk, int(item_slices),
                                        _ptr(ids, torch.int64, "ids"), _ptr(scores, torch.float32, "scores"),
                                        _ptr(ws, torch.uint8, "ws"), ws.numel(), _stream()))
    return (ids, scores) if return_scores else ids


def _check_targets(indptr, items, user_num):
    """_check_exclusion for the target CSR of full_rank_positions, whose rows must ascend STRICTLY: a duplicate target
    would be two outputs of one item."""
    if indptr.dim() != 1 or items.dim() != 1 or indptr.numel() != user_num + 1:
        raise ValueError(f"targets: indptr has {indptr.numel()} entries, the user table has {user_num} rows "
                         f"(expected {user_num + 1})")
    nnz = items.numel()
    if not bool(((indptr[1:] >= indptr[:-1]).all() & (indptr[0] == 0) & (indptr[-1] == nnz)).item()):
        raise ValueError(f"targets: indptr must rise from 0 to len(items) = {nnz}")
    if nnz > 1:
        inside = torch.ones(nnz + 1, dtype=torch.bool, device=items.device)
        inside[indptr] = False
        down, same = ((items[1:] < items[:-1]) & inside[1:nnz]).any(), ((items[1:] == items[:-1]) & inside[1:nnz]).any()
        down, same = torch.stack([down, same]).tolist()
        if down:
            raise ValueError("targets: the items of a row must be ascending (utils.user_csr / ops.build_user_csr sort them)")
        if same:
            raise ValueError("targets: a row holds the same item twice")


def full_rank_positions(P, Q, users, targets, exclude=None, biases=None, return_scores=False, return_eligible=False,
                        item_slices=0, validate=True):
    """The exact 0-based rank of every held-out item among ALL eligible items (csrc/rank_positions.hip):
    for request b = users[b] and every item t of the user's row of `targets` = (indptr int64 [U + 1], items int32
    ascending per row), the number of items outside the user's row of `exclude` whose (score, id) comes before t's in
    full_rank_users' order - bit for bit the index full_rank_users would list t at, without its cap on topk.  ->
    (out_indptr int64 [n + 1], positions int32 [T][, scores float32 [T]][, eligible int32 [n]]): request b's targets in
    row order at out_indptr[b] .. out_indptr[b + 1]; -1 (score -inf) for a target outside [0, I) or inside the exclusion
    row; eligible = the items a user can be recommended.  validate: full_rank_users' checks on users, exclude and
    targets (one read-back each; duplicate targets in a row are a ValueError); False skips them - the kernels then trust
    the ids and the indptr arrays, only compare the exclusion's contents and range-check every target id."""
    U, I = int(P.shape[0]), int(Q.shape[0])
    if P.dim() != 2 or Q.dim() != 2 or P.shape[1] != Q.shape[1]:
        raise ValueError(f"full_rank_positions: P {tuple(P.shape)} and Q {tuple(Q.shape)} need the same column count")
    dev = P.device
    users = torch.as_tensor(users).to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    n = users.numel()
    t_indptr, t_items = targets
    indptr = items = None
    if exclude is not None:
        indptr, items = exclude
        if items.numel() == 0:              # (an empty tensor has no pointer to hand over)
            items = torch.zeros(1, dtype=torch.int32, device=dev)
    if n and validate:
        lo, hi = (int(x) for x in torch.stack([users.min(), users.max()]).tolist())
        if lo < 0 or hi >= U:
            raise IndexError(f"index {hi if hi >= U else lo} is out of bounds for the user table with {U} rows")
        if exclude is not None:
            _check_exclusion(indptr, exclude[1], U)
        _check_targets(t_indptr, t_items, U)
    elif t_indptr.numel() != U + 1:
        raise ValueError(f"targets: indptr has {t_indptr.numel()} entries, the user table has {U} rows (expected {U + 1})")
    out_indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n:
        torch.cumsum(t_indptr[users + 1] - t_indptr[users], 0, out=out_indptr[1:])
    T = int(out_indptr[-1]) if n else 0
    pos = torch.empty(T, dtype=torch.int32, device=dev)
    scores = torch.empty(T, dtype=torch.float32, device=dev) if return_scores else None
    eligible = torch.empty(n, dtype=torch.int32, device=dev) if return_eligible else None
    if n and (T or return_eligible):
        if t_items.numel() == 0:
            t_items = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = _ws(lib.daisy_full_rank_positions_workspace_bytes(n, T), dev)
        bu, bi, b0 = _bias_ptrs(biases)
        dummy = pos if T else torch.zeros(1, dtype=torch.int32, device=dev)
        check(lib.daisy_full_rank_positions(_ptr(P, torch.float32, "P"), _ptr(Q, torch.float32, "Q"), bu, bi, b0, P.shape[1], I,
                                            _ptr(users, torch.int64, "users"), n, _ptr(indptr, torch.int64, "exclude indptr"),
                                            _ptr(items, torch.int32, "exclude items"),
                                            _ptr(t_indptr, torch.int64, "targets indptr"),
                                            _ptr(t_items, torch.int32, "targets items"),
                                            _ptr(out_indptr, torch.int64, "out_indptr"), T, int(item_slices),
                                            _ptr(dummy, torch.int32, "positions"), _ptr(scores, torch.float32, "scores"),
                                            _ptr(eligible, torch.int32, "eligible"), _ptr(ws, torch.uint8, "ws"), ws.numel(),
                                            _stream()))
    out = (out_indptr, pos)
    if return_scores:
        out += (scores,)
    if return_eligible:
        out += (eligible,)
    return out


POSITION_KPIS = ("precision", "recall", "hit", "mrr", "map", "ndcg", "f1", "auc", "full_auc")


def position_kpis(out_indptr, positions, gt_len, eligible, cutoffs, metrics, disc=None, disc_cum=None, per_user=False):
    """daisy_position_kpis: the per-list KPIs of ranking_kpis (and 'full_auc') at every cutoff - any K >= 1 - from
    full_rank_positions' outputs.  gt_len int64 [n] (None: the row lengths), eligible int32 [n]; disc float64 = 1 /
    log2(p + 2) and disc_cum, its running sum, for every position below the largest cutoff (needed for ndcg, built on
    the host like ranking_kpis' disc).  -> (names in slot order, per_user float64 [len(names), nc, n] or None, means
    float64 [len(names), nc])."""
    mask = 0
    for name in metrics:
        if name in ("popularity", "diversity", "coverage"):
            raise ValueError(f"'{name}' needs the ranked lists: use full_rank_users + ranking_kpis")
        if name not in POSITION_KPIS:
            raise ValueError(f"Invalid metric name {name}")
        mask |= 1 << (N.KPI_FULL_AUC if name == "full_auc" else N.KPI_IDS[name])
    names = [m for m in POSITION_KPIS if m in metrics]
    dev = positions.device
    n, nc = out_indptr.numel() - 1, len(cutoffs)
    cuts = (C.c_int32 * max(nc, 1))(*[int(k) for k in cutoffs])
    out_user = torch.empty(len(names), nc, n, dtype=torch.float64, device=dev) if per_user else None
    means = torch.empty(len(names), nc, dtype=torch.float64, device=dev)
    if "ndcg" in metrics and (disc is None or disc_cum is None or disc.numel() != disc_cum.numel()):
        raise ValueError("'ndcg' needs disc and disc_cum, of one length")
    disc_len = 0 if disc is None else disc.numel()
    if positions.numel() == 0:
        positions = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = _ws(lib.daisy_position_kpis_workspace_bytes(n, nc, mask), dev)
    check(lib.daisy_position_kpis(_ptr(out_indptr, torch.int64, "out_indptr"), _ptr(positions, torch.int32, "positions"),
                                  _ptr(gt_len, torch.int64, "gt_len"), _ptr(eligible, torch.int32, "eligible"), n, cuts, nc,
                                  _ptr(disc, torch.float64, "disc"), _ptr(disc_cum, torch.float64, "disc_cum"), disc_len, mask,
                                  _ptr(out_user, torch.float64, "per_user"), _ptr(means, torch.float64, "means"),
                                  _ptr(ws, torch.uint8, "ws"), ws.numel(), _stream()))
    return names, out_user, means


def build_user_csr(users, items, user_num):
    """get_ur (utils.py:19-34) as a device CSR: (indptr int64[U+1], sorted items int32[n])."""
    n = users.numel()
    indptr = torch.empty(user_num + 1, dtype=torch.int64, device=users.device)
    csr_items = torch.empty(n, dtype=torch.int32, device=users.device)
    ws = _ws(lib.daisy_csr_workspace_bytes(n), users.device)
    check(lib.daisy_build_user_csr(_ptr(users, torch.int32, "users"), _ptr(items, torch.int32, "items"),
                                   n, int(user_num), _ptr(indptr, torch.int64, "indptr"),
                                   _ptr(csr_items, torch.int32, "csr_items"), _ptr(ws, torch.uint8, "ws"),
                                   ws.numel(), _stream()))
    return indptr, csr_items


def sample_neg_per_user(indptr, csr_items, item_num, num_ng, seed, epoch=0):
    U = indptr.numel() - 1
    js = torch.empty(U, num_ng, dtype=torch.int32, device=indptr.device)
    check(lib.daisy_sample_neg_per_user(_ptr(indptr, torch.int64, "indptr"),
                                        _ptr(csr_items, torch.int32, "csr_items"), U, int(item_num),
                                        int(num_ng), int(seed), int(epoch), _ptr(js, torch.int32, "js"),
                                        _stream()))
    return js


POP_STREAM = 1 << 62          # Philox stream of the popularity-weighted draws (the uniform ones use `epoch`)


def sample_categorical(cdf, rows, k, seed, stream_id, out=None, col0=0):
    """k draws per row from the categorical distribution with inclusive cumulative sums `cdf` (float64 [I], device):
    the 'high-pop' / 'low-pop' share of sampler.py:76-80.  Written into out[:, col0:col0+k] (int32 [rows, ld])."""
    if out is None:
        out = torch.empty(rows, k, dtype=torch.int32, device=cdf.device)
    check(lib.daisy_sample_categorical(_ptr(cdf, torch.float64, "cdf"), cdf.numel(), int(rows), int(k), int(seed),
                                       int(stream_id), _ptr(out, torch.int32, "out"), out.shape[1], int(col0), _stream()))
    return out


def skipgram_samples(seq_items, seq_user, seq_ptr, context_window, ur_indptr, ur_items, item_num, seed, stream_id=0):
    """SkipGramNegativeSampler.sampling (sampler.py:133-155) on the device: int32 [rows, 3] (target, context, label)
    rows, element by element of the user sequences - window positives, then as many uniform negatives."""
    dev = seq_items.device
    n = seq_items.numel()
    pos = torch.arange(n, device=dev, dtype=torch.int64) - seq_ptr[seq_user.long()]
    length = (seq_ptr[1:] - seq_ptr[:-1])[seq_user.long()]
    w = int(context_window)
    cnt = torch.clamp(pos, max=w) + torch.clamp(length - 1 - pos, max=w)                 # window size of every element
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(2 * cnt, 0)
    rows = int(off[-1].item())
    out = torch.empty(rows, 3, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    if rows:
        check(lib.daisy_skipgram_samples(_ptr(seq_items, torch.int32, "seq_items"), _ptr(seq_user, torch.int32, "seq_user"),
                                         _ptr(seq_ptr, torch.int64, "seq_ptr"), _ptr(off, torch.int64, "row_offsets"), n, w,
                                         _ptr(ur_indptr, torch.int64, "ur_indptr"), _ptr(ur_items, torch.int32, "ur_items"),
                                         int(item_num), int(seed), int(stream_id), _ptr(out, torch.int32, "out"),
                                         _ptr(bad, torch.int32, "bad"), _stream()))
    if int(bad.item()):
        raise ValueError("'a' cannot be empty unless no samples are taken")      # np.random.choice on an empty complement
    return out


def expand_triples(users, items, js):
    n, num_ng = users.numel(), js.shape[1]
    out = torch.empty(n * num_ng, 3, dtype=torch.int32, device=users.device)
    check(lib.daisy_expand_triples(_ptr(users, torch.int32, "users"), _ptr(items, torch.int32, "items"),
                                   n, _ptr(js, torch.int32, "js"), num_ng,
                                   _ptr(out, torch.int32, "triples"), _stream()))
    return out


def resample_neg_per_interaction(indptr, csr_items, item_num, triples, seed, epoch=0):
    check(lib.daisy_resample_neg_per_interaction(
        _ptr(indptr, torch.int64, "indptr"), _ptr(csr_items, torch.int32, "csr_items"), int(item_num),
        _ptr(triples, torch.int32, "triples"), triples.shape[0], int(seed), int(epoch), _stream()))
    return triples


def build_candidates(indptr_test, items_test, indptr_train, items_train, users, item_num, cand_num, seed):
    """build_candidates_set (utils.py:53-85) on the device -> int64 [n_users, cand_num]."""
    users = users.to(torch.int64).contiguous()
    out = torch.empty(users.numel(), cand_num, dtype=torch.int64, device=users.device)
    check(lib.daisy_build_candidates(_ptr(indptr_test, torch.int64, "indptr_test"),
                                     _ptr(items_test, torch.int32, "items_test"),
                                     _ptr(indptr_train, torch.int64, "indptr_train"),
                                     _ptr(items_train, torch.int32, "items_train"),
                                     _ptr(users, torch.int64, "users"), users.numel(), int(item_num),
                                     int(cand_num), int(seed), _ptr(out, torch.int64, "out"), _stream()))
    return out


def randperm(n, seed, epoch=0, device="cuda"):
    perm = torch.empty(n, dtype=torch.int64, device=device)
    ws = _ws(lib.daisy_randperm_workspace_bytes(n), perm.device)
    check(lib.daisy_randperm(int(n), int(seed), int(epoch), _ptr(perm, torch.int64, "perm"),
                             _ptr(ws, torch.uint8, "ws"), ws.numel(), _stream()))
    return perm


def membench(what, table, idx, out):
    check(lib.daisy_membench(int(what), _ptr(table, torch.float32, "table"), table.shape[0],
                             table.shape[1], _ptr(idx, torch.int32, "idx"), idx.numel(),
                             _ptr(out, torch.float32, "out"), _stream()))


# ------------------------------------------------------------------------------------------------
# NeuMF (NeuMFRecommender.py) - see include/daisyrec_amd.h
# ------------------------------------------------------------------------------------------------
NEUMF_MODELS = {"NeuMF": N.NEUMF_FULL, "NeuMF-end": N.NEUMF_FULL, "GMF": N.NEUMF_GMF, "MLP": N.NEUMF_MLP}


def neumf_param_names(num_layers):
    names = ["uG", "iG", "uM", "iM"]
    for l in range(1, num_layers + 1):
        names += [f"W{l}", f"b{l}"]
    return names + ["Wp", "bp"]


def _neumf_table(tensors, num_layers):
    """dict name -> float32 device tensor  =>  daisy_neumf_params"""
    t = N.NeumfParams()
    f = torch.float32
    for k in ("uG", "iG", "uM", "iM", "Wp", "bp"):
        setattr(t, k, _ptr(tensors[k], f, k))
    for l in range(1, num_layers + 1):
        t.W[l - 1] = _ptr(tensors[f"W{l}"], f, f"W{l}")
        t.b[l - 1] = _ptr(tensors[f"b{l}"], f, f"b{l}")
    return t


class NeumfContext(_Native):
    """Activation workspace + entry points of the NeuMF path (daisy_neumf_*)."""

    _destroy = lib.daisy_neumf_ctx_destroy
    _bytes = lib.daisy_neumf_ctx_bytes

    def __init__(self, max_rows, factors, num_layers, user_num, item_num, model="NeuMF", device=None):
        if model not in NEUMF_MODELS:
            raise NotImplementedError(f"NeuMF model_name '{model}' (native: {sorted(NEUMF_MODELS)})")
        self.device = torch.device(device if device is not None else "cuda")
        self.L, self.d = int(num_layers), int(factors)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib.daisy_neumf_ctx_create(C.byref(self._h), int(max_rows), int(factors), int(num_layers),
                                             NEUMF_MODELS[model], int(user_num), int(item_num)))
        self.max_rows = int(max_rows)
        self.stats = torch.zeros(N.NEUMF_STATS_LEN, dtype=torch.float64, device=self.device)

    def set_precision(self, bf16_gemm):
        """0 / False (default): exact fp32; 1 / True: bf16-input MFMA in the MLP tower (fp32 operands rounded on the way
        into LDS); 2: activations and a copy of the weights stored as bf16 in HBM too (throughput modes)."""
        check(lib.daisy_neumf_ctx_set_precision(self._h, int(bf16_gemm)))

    def scores(self, params, users, items=None, C_=0, n=None):
        """NeuMF.forward in eval mode: see daisy_neumf_scores for the three pair layouts."""
        users = users.to(torch.int64).contiguous()
        if items is not None:
            items = items.to(torch.int64).contiguous()
            n = items.numel()
        out = torch.empty(int(n), dtype=torch.float32, device=self.device)
        tab = _neumf_table(params, self.L)
        check(lib.daisy_neumf_scores(self._h, C.byref(tab), _ptr(users, torch.int64, "users"),
                                     _ptr(items, torch.int64, "items"), int(n), int(C_),
                                     _ptr(out, torch.float32, "out"), _stream()))
        return out

    def scores_users(self, params, users, out):
        """The eval-mode scores of users [m] (int64 device) against ALL items into out float32 [m, item_num] (contiguous):
        daisy_neumf_scores_users - the forward code of `scores`, no candidate array."""
        tab = _neumf_table(params, self.L)
        check(lib.daisy_neumf_scores_users(self._h, C.byref(tab), _ptr(users, torch.int64, "users"), int(users.numel()),
                                           _ptr(out, torch.float32, "out"), _stream()))
        return out

    def step_grads(self, params, grads, u, i, j, loss_type=N.LOSS_BPR, reg_1=0.0, reg_2=0.0, dropout=0.0,
                   seed=0, gamma=1e-10):
        """NeuMF.calc_loss + backward for one batch: accumulates into `grads`, loss in stats[NST_LOSS]."""
        pt, gt = _neumf_table(params, self.L), _neumf_table(grads, self.L)
        check(lib.daisy_neumf_step_grads(self._h, C.byref(pt), C.byref(gt), _ptr(u, torch.int32, "u"),
                                         _ptr(i, torch.int32, "i"), _ptr(j, torch.int32, "j"), u.numel(),
                                         int(loss_type), float(gamma), float(reg_1), float(reg_2), float(dropout),
                                         int(seed), _ptr(self.stats, torch.float64, "stats"), _stream()))


    def fit_epoch(self, params, grads, u, i, j, batch, optim, W, g, loss_type=N.LOSS_BPR, reg_1=0.0, reg_2=0.0, dropout=0.0,
                  seed_hi=0, step0=0, gamma=1e-10):
        """One epoch of AbstractRecommender.fit's loop (:112-128) over the batches of (u, i, j), issued by the library
        (daisy_neumf_fit_epoch): step_grads + the dense optimiser `optim` on the flat vectors W / g per batch.  Advances
        optim.t by the number of steps and returns that number; the epoch's loss accumulates in stats[NST_LOSS_SUM]."""
        n = int(u.numel())
        steps = (n + int(batch) - 1) // int(batch)
        if optim.t != int(step0):
            raise ValueError(f"fit_epoch: the optimiser has taken {optim.t} steps, step0 = {step0}")
        W, g = W.view(-1), g.view(-1)
        pt, gt = _neumf_table(params, self.L), _neumf_table(grads, self.L)
        check(lib.daisy_neumf_fit_epoch(self._h, C.byref(pt), C.byref(gt), _ptr(u, torch.int32, "u"), _ptr(i, torch.int32, "i"),
                                        _ptr(j, torch.int32, "j"), n, int(batch), int(loss_type), float(gamma), float(reg_1),
                                        float(reg_2), float(dropout), int(seed_hi), int(step0), *optim.native_args(W, g),
                                        W.numel(), _ptr(self.stats, torch.float64, "stats"), _stream()))
        optim.t += steps
        return steps


def sgd_dense(W, g, lr):
    check(lib.daisy_sgd_dense(_ptr(W, torch.float32, "W"), _ptr(g, torch.float32, "g"), W.numel(), float(lr),
                              _stream()))


def topk_from_scores(scores, cands, topk):
    """argsort(descending, stable) + gather + [:topk] of every rank() (e.g. NeuMFRecommender.py:203-206)."""
    cands = cands.to(torch.int64).contiguous()
    B, Cn = cands.shape
    out = torch.empty(B, topk, dtype=torch.int64, device=scores.device)
    ws = _ws(lib.daisy_mf_rank_workspace_bytes(B, Cn), scores.device)
    check(lib.daisy_topk_from_scores(_ptr(scores.contiguous(), torch.float32, "scores"),
                                     _ptr(cands, torch.int64, "cands"), B, Cn, int(topk),
                                     _ptr(out, torch.int64, "out"), _ptr(ws, torch.uint8, "ws"), ws.numel(),
                                     _stream()))
    return out


def full_topk_from_scores(scores, topk):
    I = scores.numel()
    out = torch.empty(topk, dtype=torch.int64, device=scores.device)
    ws = _ws(lib.daisy_mf_full_rank_workspace_bytes(I), scores.device)
    check(lib.daisy_full_topk_from_scores(_ptr(scores.contiguous(), torch.float32, "scores"), I, int(topk),
                                          _ptr(out, torch.int64, "out"), _ptr(ws, torch.uint8, "ws"), ws.numel(),
                                          _stream()))
    return out


def gemm_nt_bf16(A, B):
    """C = A @ B.T with bf16 storage for A [M,K], B [N,K] and C [M,N] (fp32 accumulation on the MFMA units)."""
    M, K = A.shape
    Nn = B.shape[0]
    out = torch.empty(M, Nn, dtype=torch.bfloat16, device=A.device)
    check(lib.daisy_gemm_nt_bf16(_ptr(A, torch.bfloat16, "A"), _ptr(B, torch.bfloat16, "B"), _ptr(out, torch.bfloat16, "C"),
                                 M, Nn, K, _stream()))
    return out


def gemm_tn_bf16(At, Bt, k_chunk=2048):
    """C = At.T @ Bt for bf16 At [K,M], Bt [K,N] (the weight-gradient layout of NeuMF's precision level 2), fp32
    result, the reduction cut into k_chunk slices (fp32 atomics)."""
    K, M = At.shape
    Nn = Bt.shape[1]
    out = torch.zeros(M, Nn, dtype=torch.float32, device=At.device)
    check(lib.daisy_gemm_tn_bf16(_ptr(At, torch.bfloat16, "At"), _ptr(Bt, torch.bfloat16, "Bt"),
                                 _ptr(out, torch.float32, "C"), M, Nn, K, int(k_chunk), _stream()))
    return out


def gemm_nt(A, B, bf16=False):
    """C = A @ B.T on the MFMA tile kernels of the NeuMF tower (test / bench hook)."""
    M, K = A.shape
    Nn = B.shape[0]
    out = torch.empty(M, Nn, dtype=torch.float32, device=A.device)
    check(lib.daisy_gemm_nt(_ptr(A, torch.float32, "A"), _ptr(B, torch.float32, "B"),
                            _ptr(out, torch.float32, "C"), M, Nn, K, int(bool(bf16)), _stream()))
    return out


def gemm_case(a, b=None):
    """One product (or, with `b`, a pair in one launch) through the launcher its `N.GemmDesc` names (test hook): the
    library checks every extent against the descriptor's element counts before it launches and raises ValueError
    otherwise.  Returns the path word the launcher resolved (`N.gemm_path` decodes it).  `a.dry_run`: no GPU is touched."""
    stream = None if a.dry_run else _stream()
    check(lib.daisy_gemm_case(C.byref(a), C.byref(b) if b is not None else None, stream))
    return int(a.path)


# ------------------------------------------------------------------------------------------------
# LightGCN (LightGCNRecommender.py) - see include/daisyrec_amd.h
# ------------------------------------------------------------------------------------------------
class LgcnGraph(_Native):
    """Normalised adjacency A_hat = D^-1/2 A D^-1/2 of the user-item graph on the device
    (LightGCNRecommender.py:74-107) and the products built on it."""

    _destroy = lib.daisy_lgcn_graph_destroy
    _bytes = lib.daisy_lgcn_graph_bytes

    def __init__(self, users, items, user_num, item_num):
        users = users.to(torch.int32).contiguous()
        items = items.to(torch.int32).contiguous()
        self.device = users.device
        self.U, self.I = int(user_num), int(item_num)
        self.N = self.U + self.I
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib.daisy_lgcn_graph_create(C.byref(self._h), _ptr(users, torch.int32, "users"),
                                              _ptr(items, torch.int32, "items"), users.numel(), self.U, self.I,
                                              _stream()))
        self.nnz = int(lib.daisy_lgcn_graph_nnz(self._h))
        self._work = None

    def set_reproducible(self, flag):
        """True: row-owner products (bitwise reproducible); False (default): chunked segmented reduction."""
        check(lib.daisy_lgcn_graph_set_reproducible(self._h, int(bool(flag))))

    def coo(self):
        row = torch.empty(self.nnz, dtype=torch.int32, device=self.device)
        col = torch.empty_like(row)
        val = torch.empty(self.nnz, dtype=torch.float32, device=self.device)
        check(lib.daisy_lgcn_graph_read(self._h, _ptr(row, torch.int32, "row"), _ptr(col, torch.int32, "col"),
                                        _ptr(val, torch.float32, "val"), _stream()))
        return row, col, val

    def _scratch(self, d):
        if self._work is None or self._work.numel() < 2 * self.N * d:
            self._work = torch.empty(2 * self.N * d, dtype=torch.float32, device=self.device)
        return self._work

    def spmm(self, X, pitch=None, accumulate=False, keep=None, out=None, transpose=False):
        """Y = A_hat X.  Any of the NGCF options - a column-slice view X / out (pitch: the rows' stride, taken from the
        views), accumulate (out += A_hat X), keep=(p, seed) node dropout, transpose - goes through spmm_ex."""
        if pitch is not None or accumulate or keep is not None or out is not None or transpose:
            if pitch is not None:
                assert X.stride(0) == pitch, (X.stride(), pitch)
            return self.spmm_ex(X, out=out, accumulate=accumulate, keep=keep, transpose=transpose)
        Y = torch.empty_like(X)
        check(lib.daisy_lgcn_spmm(self._h, _ptr(X, torch.float32, "X"), _ptr(Y, torch.float32, "Y"), X.shape[1],
                                  _stream()))
        return Y

    def spmm_rows(self, X, Yrows, row_lo, row_hi):
        """Yrows[1 + r - row_lo] = (A_hat X)[r] for r in [row_lo, row_hi): `Yrows` is [row_hi-row_lo+2, d] - the
        block plus one spare row on either side (the segmented reduction may spill a partial neighbour row there)."""
        assert Yrows.shape[0] >= row_hi - row_lo + 2 and Yrows.is_contiguous()
        check(lib.daisy_lgcn_spmm_rows(self._h, _ptr(X, torch.float32, "X"), _ptr(Yrows[1:], torch.float32, "Yrows"),
                                       X.shape[1], int(row_lo), int(row_hi), _stream()))
        return Yrows[1:1 + row_hi - row_lo]

    def spmm_ex(self, X, out=None, accumulate=False, keep=None, transpose=False):
        """NGCF's product: out (=, or += with accumulate) A_hat X, where X and out may be column slices of wider
        buffers (rows contiguous; the row pitch is their stride).  keep=(p, seed): node dropout of the stored entries
        (NGCFRecommender.py:19-36), transpose: the masked matrix's transpose.  Bitwise reproducible."""
        if out is None:
            out = torch.zeros(X.shape[0], X.shape[1], dtype=torch.float32, device=X.device) if accumulate else \
                torch.empty(X.shape[0], X.shape[1], dtype=torch.float32, device=X.device)
        assert X.shape[0] == self.N and out.shape == X.shape, (X.shape, out.shape, self.N)
        p, seed = keep if keep is not None else (0.0, 0)
        xp, ldx = _rows(X, "X")
        yp, ldy = _rows(out, "out")
        check(lib.daisy_lgcn_spmm_ex(self._h, xp, ldx, yp, ldy, X.shape[1], int(bool(accumulate)), float(p),
                                     int(seed) & (2 ** 64 - 1), int(bool(transpose)), _stream()))
        return out

    def propagate(self, E0, num_layers, out=None):
        """LightGCN.forward (LightGCNRecommender.py:117-129): mean_k A_hat^k E0, [N, d]."""
        out = torch.empty_like(E0) if out is None else out
        w = self._scratch(E0.shape[1])
        check(lib.daisy_lgcn_propagate(self._h, _ptr(E0, torch.float32, "E0"), E0.shape[1], int(num_layers),
                                       _ptr(w, torch.float32, "work"), _ptr(out, torch.float32, "out"), _stream()))
        return out

    def backprop(self, G, num_layers, dE0):
        """dE0 += 1/(L+1) sum_k A_hat^k G (the transpose of propagate; A_hat is symmetric)."""
        w = self._scratch(G.shape[1])
        check(lib.daisy_lgcn_backprop(self._h, _ptr(G, torch.float32, "G"), G.shape[1], int(num_layers),
                                      _ptr(w, torch.float32, "work"), _ptr(dE0, torch.float32, "dE0"), _stream()))


_LGCN_REG_WS = {}


def lgcn_reg_grad(E0, u, i, j, user_num, pointwise, reg_1, reg_2, stats, dE0):
    N = E0.shape[0]
    key = (E0.device, N)
    ws = _LGCN_REG_WS.get(key)            # int32 occurrence counts, kept all-zero between calls by the kernels
    if ws is None:
        ws = _LGCN_REG_WS[key] = torch.zeros(2 * N, dtype=torch.int32, device=E0.device)
    check(lib.daisy_lgcn_reg_grad(_ptr(E0, torch.float32, "E0"), _ptr(u, torch.int32, "u"), _ptr(i, torch.int32, "i"),
                                  _ptr(j, torch.int32, "j"), u.numel(), int(user_num), int(N - user_num), E0.shape[1],
                                  int(bool(pointwise)), float(reg_1), float(reg_2), _ptr(stats, torch.float64, "stats"),
                                  _ptr(ws, torch.int32, "count_ws"), _ptr(dE0, torch.float32, "dE0"), _stream()))


def axpby(x, a, b, y, zero_x=False):
    """y = a*x + b*y (and x = 0 when zero_x)."""
    check(lib.daisy_axpby_f32(_ptr(x, torch.float32, "x"), float(a), float(b), _ptr(y, torch.float32, "y"), y.numel(),
                              int(bool(zero_x)), _stream()))


def csr_row_sum(indptr, cols, X, out):
    """out[r] = sum of X[cols[e]] over the CSR row r (rows without entries untouched)."""
    check(lib.daisy_csr_row_sum(_ptr(indptr, torch.int64, "indptr"), _ptr(cols, torch.int32, "cols"),
                                _ptr(X, torch.float32, "X"), indptr.numel() - 1, X.shape[1],
                                _ptr(out, torch.float32, "out"), _stream()))


# ---- NGCF (csrc/ngcf.hip; NGCFRecommender.py:38-172) ------------------------------------------------------------------
NGCF_MAX_WIDTH, NGCF_NODE_STREAM, NGCF_MESS_STREAM = N.NGCF_MAX_WIDTH, N.NGCF_NODE_STREAM, N.NGCF_MESS_STREAM


def dropout_mask(seed, stream_id, n, p, device="cuda"):
    """uint8[n] keep bits of dropout stream `stream_id` (the test hook of the device masks)."""
    out = torch.empty(int(n), dtype=torch.uint8, device=device)
    check(lib.daisy_dropout_mask(int(seed) & (2 ** 64 - 1), int(stream_id), int(n), float(p),
                                 _ptr(out, torch.uint8, "out"), _stream()))
    return out


def ngcf_ws_bytes(n, d_in, d_out):
    return int(lib.daisy_ngcf_ws_bytes(int(n), int(d_in), int(d_out)))


def ngcf_layer_forward(E, X, W1, b1, W2, b2, Y, norm, mess_p=0.0, seed=0, layer=0):
    """One BiGNN layer + LeakyReLU + message dropout + F.normalize (NGCFRecommender.py:38-60,163-167): Y and norm are
    written.  E ([N, d_in]) and Y ([N, d_out]) may be column slices of the concat buffer; X = A_hat_drop E."""
    n, d_in = E.shape
    d_out = Y.shape[1]
    ep, lde = _rows(E, "E")
    yp, ldy = _rows(Y, "Y")
    check(lib.daisy_ngcf_layer_forward(ep, lde, _ptr(X, torch.float32, "X"), _ptr(W1, torch.float32, "W1"),
                                       _ptr(b1, torch.float32, "b1"), _ptr(W2, torch.float32, "W2"),
                                       _ptr(b2, torch.float32, "b2"), yp, ldy, _ptr(norm, torch.float32, "norm"), n,
                                       d_in, d_out, float(mess_p), int(seed) & (2 ** 64 - 1), int(layer), _stream()))
    return Y


def ngcf_layer_backward(dY, Y, norm, E, X, W1, W2, dE, dX, ws, mess_p=0.0, seed=0, layer=0, gprev=None):
    """The layer's backward pass: dE = gprev + dS + dT * X, dX = dS + dT * E (the caller adds A_hat_drop^T dX to dE)
    and the weight-gradient partials in ws (uint8 or float32 of ngcf_ws_bytes; ngcf_wgrad_reduce sums them)."""
    n, d_in = E.shape
    d_out = Y.shape[1]
    dp, ldd = _rows(dY, "dY")
    yp, ldy = _rows(Y, "Y")
    ep, lde = _rows(E, "E")
    gp, ldg = _rows(gprev, "gprev") if gprev is not None else (None, 0)
    check(lib.daisy_ngcf_layer_backward(dp, ldd, yp, ldy, _ptr(norm, torch.float32, "norm"), ep, lde,
                                        _ptr(X, torch.float32, "X"), _ptr(W1, torch.float32, "W1"),
                                        _ptr(W2, torch.float32, "W2"), gp, ldg, _ptr(dE, torch.float32, "dE"),
                                        _ptr(dX, torch.float32, "dX"), C.c_void_p(ws.data_ptr()), n, d_in, d_out,
                                        float(mess_p), int(seed) & (2 ** 64 - 1), int(layer), _stream()))


def ngcf_wgrad_reduce(ws, n, d_in, d_out, dW1, db1, dW2, db2):
    """dW1, dW2, db1, db2 += the backward pass's partials, summed in a fixed order."""
    check(lib.daisy_ngcf_wgrad_reduce(C.c_void_p(ws.data_ptr()), int(n), int(d_in), int(d_out),
                                      _ptr(dW1, torch.float32, "dW1"), _ptr(db1, torch.float32, "db1"),
                                      _ptr(dW2, torch.float32, "dW2"), _ptr(db2, torch.float32, "db2"), _stream()))


# ---- NFM (csrc/nfm.hip; NFMRecommender.py:15-209) ---------------------------------------------------------------------
def _nfm_table(t, num_layers, batch_norm):
    """daisy_nfm_params from a dict: P, Q, ub, ib, bias, W1.., b1.., wp and (batch_norm) bn_w0.., bn_b0.."""
    f = torch.float32
    p = N.NfmParams()
    for k in ("P", "Q", "ub", "ib", "bias", "wp"):
        setattr(p, k, _ptr(t[k], f, k))
    for l in range(1, num_layers + 1):
        p.W[l - 1] = _ptr(t[f"W{l}"], f, f"W{l}")
        p.b[l - 1] = _ptr(t[f"b{l}"], f, f"b{l}")
    if batch_norm:
        for s in range(num_layers + 1):
            p.bn_w[s] = _ptr(t[f"bn_w{s}"], f, f"bn_w{s}")
            p.bn_b[s] = _ptr(t[f"bn_b{s}"], f, f"bn_b{s}")
    return p


def _nfm_bn(bn, num_layers):
    """daisy_nfm_bn_state from a list of (running_mean, running_var, num_batches_tracked) per stage (None: no BN)."""
    st = N.NfmBnState()
    if bn is None:
        return st
    for s in range(num_layers + 1):
        m, v, n = bn[s]
        st.mean[s] = _ptr(m, torch.float32, f"running_mean{s}")
        st.var[s] = _ptr(v, torch.float32, f"running_var{s}")
        st.nbt[s] = _ptr(n, torch.int64, f"num_batches_tracked{s}")
    return st


class NfmContext(_Native):
    """Activation workspace + entry points of the NFM path (daisy_nfm_*)."""

    _destroy = lib.daisy_nfm_ctx_destroy
    _bytes = lib.daisy_nfm_ctx_bytes

    def __init__(self, max_rows, factors, num_layers, act, batch_norm, user_num, item_num, device=None):
        self.device = torch.device(device if device is not None else "cuda")
        self.L, self.d, self.bn = int(num_layers), int(factors), bool(batch_norm)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib.daisy_nfm_ctx_create(C.byref(self._h), int(max_rows), int(factors), int(num_layers),
                                           N.NFM_ACT.get(act, 0) if isinstance(act, str) else int(act), int(bool(batch_norm)),
                                           int(user_num), int(item_num)))
        self.max_rows = int(max_rows)
        self.stats = torch.zeros(N.NFM_STATS_LEN, dtype=torch.float64, device=self.device)

    def set_path(self, path):
        """'auto' (the layered step), 'small' (the one-workgroup step, B <= NFM_SMALL_MAX_B) or 'layered': same bits."""
        check(lib.daisy_nfm_ctx_set_path(self._h, N.NFM_PATHS[path]))

    def scores(self, params, bn, users, items=None, C_=0, n=None, train=False, dropout=0.0, seed=0):
        """NFM.forward over n pairs (daisy_nfm_scores' three pair layouts); train: training-mode BatchNorm / dropout."""
        users = users.to(torch.int64).contiguous()
        if items is not None:
            items = items.to(torch.int64).contiguous()
            n = items.numel()
        out = torch.empty(int(n), dtype=torch.float32, device=self.device)
        pt, bt = _nfm_table(params, self.L, self.bn), _nfm_bn(bn, self.L)
        check(lib.daisy_nfm_scores(self._h, C.byref(pt), C.byref(bt), _ptr(users, torch.int64, "users"),
                                   _ptr(items, torch.int64, "items"), int(n), int(C_), int(bool(train)), float(dropout),
                                   int(seed) & (2 ** 64 - 1), _ptr(out, torch.float32, "out"), _stream()))
        return out

    def scores_users(self, params, bn, users, out):
        """The eval-mode scores of users [m] (int64 device) against ALL items into out float32 [m, item_num] (contiguous):
        daisy_nfm_scores_users - the kernel of `scores`, no candidate array; the running statistics are only read."""
        pt, bt = _nfm_table(params, self.L, self.bn), _nfm_bn(bn, self.L)
        check(lib.daisy_nfm_scores_users(self._h, C.byref(pt), C.byref(bt), _ptr(users, torch.int64, "users"),
                                         int(users.numel()), _ptr(out, torch.float32, "out"), _stream()))
        return out

    def step_grads(self, params, grads, bn, u, i, j, loss_type=N.LOSS_BPR, reg_1=0.0, reg_2=0.0, dropout=0.0, seed=0,
                   gamma=1e-10):
        """NFM.calc_loss + backward for one batch: accumulates into `grads`, updates `bn`; loss in stats[NFST_LOSS]."""
        pt, gt, bt = _nfm_table(params, self.L, self.bn), _nfm_table(grads, self.L, self.bn), _nfm_bn(bn, self.L)
        check(lib.daisy_nfm_step_grads(self._h, C.byref(pt), C.byref(gt), C.byref(bt), _ptr(u, torch.int32, "u"),
                                       _ptr(i, torch.int32, "i"), _ptr(j, torch.int32, "j"), u.numel(), int(loss_type),
                                       float(gamma), float(reg_1), float(reg_2), float(dropout), int(seed) & (2 ** 64 - 1),
                                       _ptr(self.stats, torch.float64, "stats"), _stream()))

    def fit_epoch(self, params, grads, bn, u, i, j, batch, optim, W, g, loss_type=N.LOSS_BPR, reg_1=0.0, reg_2=0.0,
                  dropout=0.0, seed_hi=0, step0=0, gamma=1e-10):
        """One epoch of AbstractRecommender.fit's loop issued by the library (daisy_nfm_fit_epoch): step_grads + the
        dense optimiser per batch.  step0: the steps taken before (the dropout key of step k is seed_hi | (step0 + k));
        Adam's bias correction counts optim.t.  Advances optim.t by the number of steps and returns it; the epoch's
        loss accumulates in stats[NFST_LOSS_SUM]."""
        n = int(u.numel())
        steps = (n + int(batch) - 1) // int(batch)
        W, g = W.view(-1), g.view(-1)
        pt, gt, bt = _nfm_table(params, self.L, self.bn), _nfm_table(grads, self.L, self.bn), _nfm_bn(bn, self.L)
        check(lib.daisy_nfm_fit_epoch(self._h, C.byref(pt), C.byref(gt), C.byref(bt), _ptr(u, torch.int32, "u"),
                                      _ptr(i, torch.int32, "i"), _ptr(j, torch.int32, "j"), n, int(batch), int(loss_type),
                                      float(gamma), float(reg_1), float(reg_2), float(dropout), int(seed_hi) & (2 ** 64 - 1),
                                      int(step0), int(optim.t), *optim.native_args(W, g), W.numel(),
                                      _ptr(self.stats, torch.float64, "stats"), _stream()))
        optim.t += steps
        return steps


# ---- Multi-VAE (csrc/vae.hip; VAECFRecommender.py) ---------------------------------------------------------------------
def vae_history_csr(history_item_id, history_item_value, item_num):
    """The user rows of R as AERecommender.get_user_rating_matrix builds them (AbstractRecommender.py:147-158), as a
    CSR: (row_ptr int64 [U + 1], col int32 [nnz], val float32 [nnz]), items ascending within a row.  index_put_ without
    accumulation keeps the LAST write of an item in a row - the padding (item 0, value 0) that follows every row shorter
    than the longest erases the row's item 0 - and entries whose value is 0 are dropped (they add nothing to R, its
    norm or the encoder).  Built once per model with torch ops (off the hot path), on the device of the inputs."""
    ids = torch.as_tensor(history_item_id).to(torch.int64)
    vals = torch.as_tensor(history_item_value).to(ids.device, torch.float32)
    if ids.dim() != 2 or vals.shape != ids.shape:
        raise ValueError(f"history_item_id / history_item_value: expected two [U, L] tensors, got {tuple(ids.shape)} and "
                         f"{tuple(vals.shape)}")
    U, L = ids.shape
    I = int(item_num)
    if ids.numel() and (int(ids.min()) < -I or int(ids.max()) >= I):
        raise IndexError(f"index out of range: history item ids must lie in [0, {I})")
    ids = torch.where(ids < 0, ids + I, ids)                   # (index_put_ wraps negative indices)
    dev = ids.device
    user = torch.arange(U, device=dev, dtype=torch.int64).repeat_interleave(L)
    pos = torch.arange(L, device=dev, dtype=torch.int64).repeat(U)
    item, v = ids.reshape(-1), vals.reshape(-1)
    # (user, item) ascending, the last position of every pair last: it is the write that stays
    order = torch.argsort((user * I + item) * max(L, 1) + pos)
    ui = (user * I + item)[order]
    last = torch.ones_like(ui, dtype=torch.bool)
    if ui.numel() > 1:
        last[:-1] = ui[1:] != ui[:-1]
    keep = order[last]
    keep = keep[v[keep] != 0]
    row = user[keep]
    counts = torch.bincount(row, minlength=U) if row.numel() else torch.zeros(U, dtype=torch.int64, device=dev)
    row_ptr = torch.zeros(U + 1, dtype=torch.int64, device=dev)
    row_ptr[1:] = torch.cumsum(counts, 0)
    return row_ptr, item[keep].to(torch.int32).contiguous(), v[keep].contiguous()


class VaeContext(_Native):
    """Workspace + entry points of the Multi-VAE path (daisy_vae_*): layer widths, the batch capacity and the flat
    parameter layout (encoder.0.weight item-major)."""

    _destroy = lib.daisy_vae_ctx_destroy
    _bytes = lib.daisy_vae_ctx_bytes

    def __init__(self, max_batch, max_entries, item_num, hidden, latent_dim, device=None):
        self.device = torch.device(device if device is not None else "cuda")
        self.hidden = [int(h) for h in hidden]
        hid = (C.c_int32 * max(len(self.hidden), 1))(*self.hidden)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib.daisy_vae_ctx_create(C.byref(self._h), int(max_batch), int(max_entries), int(item_num),
                                           len(self.hidden), hid, int(latent_dim)))
        self.max_batch, self.max_entries, self.item_num = int(max_batch), int(max_entries), int(item_num)
        self.stats = torch.zeros(N.VAE_STATS_LEN, dtype=torch.float64, device=self.device)

    @property
    def param_count(self):
        return int(lib.daisy_vae_param_count(self._h))

    @staticmethod
    def _csr(csr):
        row_ptr, col, val = csr
        return (_ptr(row_ptr, torch.int64, "row_ptr"), _ptr(col, torch.int32, "col"), _ptr(val, torch.float32, "val"),
                row_ptr.numel() - 1)

    def step_grads(self, W, g, csr, users, n_entries, keep=None, eps=None, train=True, dropout=0.5, anneal=0.0, seed=0):
        """VAECF.calc_loss + backward for users [B] (int64 device): gradients into g (zero on entry), the loss into
        stats[VST_LOSS].  keep: uint8 [n_entries] / eps: float32 [B, lat // 2] (None: the device hash)."""
        rp, cp, vp, U = self._csr(csr)
        users = users.to(torch.int64).contiguous()
        check(lib.daisy_vae_step_grads(self._h, _ptr(W, torch.float32, "W"), _ptr(g, torch.float32, "g"), rp, cp, vp, U,
                                       _ptr(users, torch.int64, "users"), users.numel(), int(n_entries),
                                       _ptr(keep, torch.uint8, "keep"), _ptr(eps, torch.float32, "eps"), int(bool(train)),
                                       float(dropout), float(anneal), int(seed) & (2 ** 64 - 1),
                                       _ptr(self.stats, torch.float64, "stats"), _stream()))

    def fit_epoch(self, W, g, csr, users, batch, entries, optim, dropout, anneal_cap, total_anneal_steps, update0,
                  seed_hi=0, step0=0):
        """One epoch of AbstractRecommender.fit's loop issued by the library (daisy_vae_fit_epoch).  users: int64 device
        [n] in epoch order; entries: the history entries of every batch (host).  Advances optim.t and returns the
        number of steps; the losses accumulate in stats[VST_LOSS_SUM]."""
        rp, cp, vp, U = self._csr(csr)
        n = int(users.numel())
        steps = (n + int(batch) - 1) // int(batch)
        ent = (C.c_int64 * steps)(*[int(x) for x in entries])
        W, g = W.view(-1), g.view(-1)
        f = torch.float32
        check(lib.daisy_vae_fit_epoch(self._h, _ptr(W, f, "W"), _ptr(g, f, "g"), rp, cp, vp, U,
                                      _ptr(users, torch.int64, "users"), n, int(batch), ent, float(dropout),
                                      float(anneal_cap), int(total_anneal_steps), int(update0), int(seed_hi) & (2 ** 64 - 1),
                                      int(step0), int(optim.t), *optim.native_args(W),
                                      _ptr(self.stats, torch.float64, "stats"), _stream()))
        optim.t += steps
        return steps

    def scores(self, W, csr, users, n_entries, items=None, train=False, dropout=0.0, seed=0, keep=None, eps=None, out=None):
        """VAECF.forward's scores of users [B]: [B, item_num], or [B, C] for candidates items [B, C] (int64).  out: a
        contiguous float32 [B, item_num] (or [B, C]) tensor to write into instead of a new one."""
        rp, cp, vp, U = self._csr(csr)
        users = users.to(torch.int64).contiguous()
        B = users.numel()
        if items is not None:
            items = items.to(torch.int64).contiguous()
            Cn = items.shape[1]
        else:
            Cn = 0
        shape = (B, Cn if items is not None else self.item_num)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != shape:
            raise ValueError(f"out: expected {shape}, got {tuple(out.shape)}")
        check(lib.daisy_vae_scores(self._h, _ptr(W, torch.float32, "W"), rp, cp, vp, U, _ptr(users, torch.int64, "users"), B,
                                   int(n_entries), _ptr(items, torch.int64, "items"), int(Cn), _ptr(keep, torch.uint8, "keep"),
                                   _ptr(eps, torch.float32, "eps"), int(bool(train)), float(dropout),
                                   int(seed) & (2 ** 64 - 1), _ptr(out, torch.float32, "out"), _stream()))
        return out


# ---- SLiM (csrc/slim.hip; SLiMRecommender.py) --------------------------------------------------------------------------
def slim_csr(users, items, ratings, user_num, item_num):
    """X of SLiM._convert_df (SLiMRecommender.py:148-157) as a CSR on the device of the inputs: (row_ptr int64 [U + 1],
    col int32, val float32), items ascending within a row, duplicate (user, item) pairs summed in the order given (what
    the COO -> CSC conversion does).  Built once per fit with torch ops (off the hot path); ids must be in range."""
    users = torch.as_tensor(users).reshape(-1).to(torch.int64)
    dev = users.device
    items = torch.as_tensor(items).reshape(-1).to(dev, torch.int64)
    vals = torch.as_tensor(ratings).reshape(-1).to(dev, torch.float64)
    U, I = int(user_num), int(item_num)
    key, order = torch.sort(users * I + items, stable=True)
    vals = vals[order]
    uniq, inverse, counts = torch.unique_consecutive(key, return_inverse=True, return_counts=True)
    start = torch.cumsum(counts, 0) - counts
    pos = torch.arange(key.numel(), device=dev, dtype=torch.int64) - start[inverse]
    acc = torch.zeros(uniq.numel(), dtype=torch.float64, device=dev)
    for r in range(int(counts.max()) if counts.numel() else 0):     # the r-th occurrence of every pair: distinct targets
        sel = pos == r
        acc[inverse[sel]] += vals[sel]
    row = uniq // I
    per_row = torch.bincount(row, minlength=U) if row.numel() else torch.zeros(U, dtype=torch.int64, device=dev)
    row_ptr = torch.zeros(U + 1, dtype=torch.int64, device=dev)
    row_ptr[1:] = torch.cumsum(per_row, 0)
    return row_ptr, (uniq % I).to(torch.int32).contiguous(), acc.to(torch.float32).contiguous()


def _slim_csr_ptrs(csr):
    row_ptr, col, val = csr
    if col.numel() == 0:          # no interaction at all: the entry points still want two readable arrays
        col, val = col.new_zeros(1), val.new_zeros(1)
    return (_ptr(row_ptr, torch.int64, "row_ptr"), _ptr(col, torch.int32, "col"), _ptr(val, torch.float32, "val"),
            row_ptr.numel() - 1)


def slim_gram(csr, item_num, tile_rows=0, offered_bytes=None):
    """G = X^T X, float32 [I, I] (daisy_slim_gram): user blocks of tile_rows rows (0: the default) through the fp32 MFMA
    product, added in block order.  offered_bytes: what G and the workspace may take together (default: the device's
    free memory); a problem that does not fit is refused before anything is allocated."""
    rp, cp, vp, U = _slim_csr_ptrs(csr)
    I = int(item_num)
    dev = csr[0].device
    if offered_bytes is None:
        with torch.cuda.device(dev):
            offered_bytes = torch.cuda.mem_get_info()[0]
    check(lib.daisy_slim_gram_fits(U, I, int(tile_rows), int(offered_bytes)))
    ws = _ws(lib.daisy_slim_gram_workspace_bytes(U, I, int(tile_rows)), dev)
    G = torch.empty(I, I, dtype=torch.float32, device=dev)
    check(lib.daisy_slim_gram(rp, cp, vp, U, I, _ptr(G, torch.float32, "G"), _ptr(ws, torch.uint8, "ws"), ws.numel(),
                              _stream()))
    return G


def slim_fit(G, n_users, alpha, l1_ratio, topk, tol=1e-4, max_iter=100, col0=0, ncols=None, path="auto", moves=None):
    """The elastic nets of the columns [col0, col0 + ncols) of G (daisy_slim_cd) -> (count int32 [ncols], rows int32
    [ncols, topk], vals float32 [ncols, topk], sweeps int32 [ncols], gap float64 [ncols]); the kept pairs of a column by
    descending value, then ascending row.  moves (int64 [ncols], optional): gets every column's count of coordinate updates
    that changed a value (each read one row of G)."""
    I = int(G.shape[0])
    if G.dim() != 2 or G.shape[1] != I:
        raise ValueError(f"G: expected a square matrix, got {tuple(G.shape)}")
    ncols = I - int(col0) if ncols is None else int(ncols)
    dev, k = G.device, int(topk)
    count = torch.empty(max(ncols, 0), dtype=torch.int32, device=dev)
    rows = torch.empty(max(ncols, 0), max(k, 0), dtype=torch.int32, device=dev)
    vals = torch.empty(max(ncols, 0), max(k, 0), dtype=torch.float32, device=dev)
    sweeps = torch.empty(max(ncols, 0), dtype=torch.int32, device=dev)
    gap = torch.empty(max(ncols, 0), dtype=torch.float64, device=dev)
    p = N.SLIM_PATHS[path]
    ws = _ws(lib.daisy_slim_cd_workspace_bytes(I, max(ncols, 0), p), dev)
    check(lib.daisy_slim_cd(_ptr(G, torch.float32, "G"), I, int(n_users), float(alpha), float(l1_ratio), float(tol),
                            int(max_iter), k, int(col0), ncols, _ptr(count, torch.int32, "count"),
                            _ptr(rows, torch.int32, "rows"), _ptr(vals, torch.float32, "vals"),
                            _ptr(sweeps, torch.int32, "sweeps"), _ptr(gap, torch.float64, "gap"),
                            _ptr(moves, torch.int64, "moves"), p,
                            _ptr(ws, torch.uint8, "ws"), ws.numel(), _stream()))
    return count, rows, vals, sweeps, gap


def slim_columns(count, rows, vals, item_num):
    """The kept pairs of slim_fit for ALL item_num columns as the column form daisy_slim_scores reads: (w_ptr int64
    [I + 1], w_row int32 ascending within a column, w_val float32; never empty: one unused slot when nothing is kept).
    Torch ops, once per fit."""
    ncols, k = rows.shape
    if ncols != int(item_num):
        raise ValueError(f"slim_columns: {ncols} columns given, item_num={item_num} (the slabs of every column, concatenated)")
    dev = rows.device
    taken = torch.arange(k, device=dev).unsqueeze(0) < count.to(torch.int64).unsqueeze(1)
    colid = torch.arange(ncols, device=dev, dtype=torch.int64).unsqueeze(1).expand(ncols, k)[taken]
    r, v = rows[taken].to(torch.int64), vals[taken]
    order = torch.argsort(colid * max(ncols, 1) + r)
    w_ptr = torch.zeros(ncols + 1, dtype=torch.int64, device=dev)
    w_ptr[1:] = torch.cumsum(count.to(torch.int64), 0)
    w_row, w_val = r[order].to(torch.int32).contiguous(), v[order].contiguous()
    if w_row.numel() == 0:
        w_row, w_val = w_row.new_zeros(1), w_val.new_zeros(1)
    return w_ptr, w_row, w_val


# _slim_operands, _psvd_operands, _ease_operands, _knn_operands: a family's shape checks, once -> (the
# leading arguments of its C entries in their order, the user count, the item count, the device, the score dtype of its
# full-rank entries, whether its entries end in a `path`); _f64_rank, _f64_full_rank_users and _f64_full_rank_positions
# make the request of each kind and call the entry on them.
def _slim_operands(csr, W, item_num):
    rp, cp, vp, U = _slim_csr_ptrs(csr)
    w_ptr, w_row, w_val = W
    I = int(item_num)
    lead = (rp, cp, vp, U, I, _ptr(w_ptr, torch.int64, "w_ptr"), _ptr(w_row, torch.int32, "w_row"),
            _ptr(w_val, torch.float32, "w_val"))
    return lead, U, I, w_ptr.device, torch.float32, True


def _candidates(users, items, n_items):
    """The request of a *_rank / slim_scores call: (users int64 [B], B, items int64 [B, C] or None, C - n_items for None)."""
    users = users.to(torch.int64).contiguous()
    B = users.numel()
    if items is None:
        return users, B, None, n_items
    items = items.to(torch.int64).contiguous()
    if items.dim() != 2 or items.shape[0] != B:
        raise ValueError(f"items: expected [{B}, C], got {tuple(items.shape)}")
    return users, B, items, int(items.shape[1])


def slim_scores(csr, W, item_num, users, items=None, path="auto"):
    """Rows of A_tilde = X W for users [B] (daisy_slim_scores): float32 [B, C] at the candidates items [B, C] (int64), or
    [B, item_num].  W: slim_columns' triple."""
    lead, _, I, _, _, _ = _slim_operands(csr, W, item_num)
    users, B, items, Cn = _candidates(users, items, I)
    out = torch.empty(B, Cn, dtype=torch.float32, device=users.device)
    check(lib.daisy_slim_scores(*lead, _ptr(users, torch.int64, "users"), B, _ptr(items, torch.int64, "items"),
                                0 if items is None else Cn, _ptr(out, torch.float32, "out"), N.SLIM_PATHS[path], _stream()))
    return out


def _f64_rank(fn, operands, users, items, topk, path=None):
    """What ease_rank, knn_rank and psvd_rank share: the request, the outputs and the call of `fn`, the family's
    daisy_*_rank.  -> (scores float64 [B, C], ids int64 [B, min(topk, C)] or None)"""
    lead, _, I, dev, _, has_path = operands
    users, B, items, Cn = _candidates(users, items, I)
    scores = torch.empty(B, Cn, dtype=torch.float64, device=dev)
    kk = min(int(topk), Cn)
    ids = torch.empty(B, kk, dtype=torch.int64, device=dev) if kk > 0 else None
    check(fn(*lead, _ptr(users, torch.int64, "users"), B, _ptr(items, torch.int64, "items"), Cn, kk,
             _ptr(scores, torch.float64, "scores"), _ptr(ids, torch.int64, "ids"),
             *((N.SLIM_PATHS[path],) if has_path else ()), _stream()))
    return scores, ids


# ---- PureSVD (csrc/puresvd.hip; PureSVDRecommender.py) --------------------------------------------------------
def _f64(t, name, dim=2):
    if not isinstance(t, torch.Tensor) or t.dim() != dim:
        raise TypeError(f"{name}: expected a {dim}-D torch.Tensor")
    return _ptr(t, torch.float64, name)


def psvd_spmm(csr, n_cols, X):
    """Y [n_rows, c] = A X, float64 (daisy_psvd_spmm): A the CSR triple of slim_csr ([n_rows, n_cols]), X float64
    [n_cols, c]; a row's non-zeros are accumulated in stored order."""
    rp, cp, vp, n_rows = _slim_csr_ptrs(csr)
    xp = _f64(X, "X")
    if X.shape[0] != int(n_cols):
        raise ValueError(f"X: expected [{int(n_cols)}, c], got {tuple(X.shape)}")
    c = int(X.shape[1])
    Y = torch.empty(n_rows, c, dtype=torch.float64, device=X.device)
    check(lib.daisy_psvd_spmm(rp, cp, vp, n_rows, int(n_cols), xp, c, _ptr(Y, torch.float64, "Y"), _stream()))
    return Y


def psvd_gram(Y, block_rows=0):
    """G [c, c] = Y^T Y, float64 (daisy_psvd_gram): blocks of block_rows rows (0: the default) on the fp64 MFMA, their
    partial products added in block order."""
    yp = _f64(Y, "Y")
    n, c = int(Y.shape[0]), int(Y.shape[1])
    ws = _ws(lib.daisy_psvd_gram_workspace_bytes(n, c, int(block_rows)), Y.device)
    G = torch.empty(c, c, dtype=torch.float64, device=Y.device)
    check(lib.daisy_psvd_gram(yp, n, c, _ptr(G, torch.float64, "G"), int(block_rows), _ptr(ws, torch.uint8, "ws"), ws.numel(),
                              _stream()))
    return G


def psvd_chol(G, n):
    """(R, Rinv, dropped) of daisy_psvd_chol: the upper R with R^T R = G that drops dependent columns (pivot not
    > 64 n eps G_jj), the inverse of R restricted to the kept columns, and the dropped count as an int32 device tensor."""
    gp = _f64(G, "G")
    c = int(G.shape[0])
    if G.shape[1] != c:
        raise ValueError(f"G: expected a square matrix, got {tuple(G.shape)}")
    R, Rinv = torch.empty_like(G), torch.empty_like(G)
    dropped = torch.zeros(1, dtype=torch.int32, device=G.device)
    check(lib.daisy_psvd_chol(gp, c, int(n), _ptr(R, torch.float64, "R"), _ptr(Rinv, torch.float64, "Rinv"),
                              _ptr(dropped, torch.int32, "dropped"), _stream()))
    return R, Rinv, dropped


def psvd_gemm(Y, T):
    """Y [n, c] T [c, c2] -> float64 [n, c2] on the fp64 MFMA (daisy_psvd_gemm)."""
    yp, tp = _f64(Y, "Y"), _f64(T, "T")
    n, c, c2 = int(Y.shape[0]), int(Y.shape[1]), int(T.shape[1])
    if T.shape[0] != c:
        raise ValueError(f"T: expected [{c}, c2], got {tuple(T.shape)}")
    out = torch.empty(n, c2, dtype=torch.float64, device=Y.device)
    check(lib.daisy_psvd_gemm(yp, tp, _ptr(out, torch.float64, "out"), n, c, c2, _stream()))
    return out


def psvd_orthonormalize(Y, block_rows=0):
    """Cholesky-QR2 of Y [n, c] -> (Q, R, dropped): two rounds of Gram, Cholesky, Y R^-1; R = R2 R1.  For the kept columns
    Q R = Y and Q^T Q = I; a dropped (dependent) column of Q is exactly zero.  dropped: int32 device tensor [1]."""
    n = int(Y.shape[0])
    R1, Ri1, _ = psvd_chol(psvd_gram(Y, block_rows), n)
    Q1 = psvd_gemm(Y, Ri1)
    R2, Ri2, dropped = psvd_chol(psvd_gram(Q1, block_rows), n)
    return psvd_gemm(Q1, Ri2), psvd_gemm(R2, R1), dropped


def psvd_jacobi(A, max_sweeps=60):
    """One-sided Jacobi SVD of A [c, c] = U diag(s) V^T (daisy_psvd_jacobi) -> (U, s, V, info): s non-increasing, info an
    int32 device tensor [status (N.PSVD_CONVERGED / N.PSVD_NOT_CONVERGED), sweeps]."""
    ap = _f64(A, "A")
    c = int(A.shape[0])
    if A.shape[1] != c:
        raise ValueError(f"A: expected a square matrix, got {tuple(A.shape)}")
    U, V = torch.empty_like(A), torch.empty_like(A)
    s = torch.empty(c, dtype=torch.float64, device=A.device)
    info = torch.zeros(2, dtype=torch.int32, device=A.device)
    ws = _ws(lib.daisy_psvd_jacobi_workspace_bytes(c), A.device)
    check(lib.daisy_psvd_jacobi(ap, c, int(max_sweeps), _ptr(U, torch.float64, "U"), _ptr(s, torch.float64, "s"),
                                _ptr(V, torch.float64, "V"), _ptr(info, torch.int32, "info"), _ptr(ws, torch.uint8, "ws"),
                                ws.numel(), _stream()))
    return U, s, V, info


def psvd_fit(csr, csr_t, omega, n_iter, max_sweeps=60):
    """randomized_svd's sequence for M [n, m] (csr: M, csr_t: M^T, both slim_csr triples) from the test matrix omega
    float64 [m, r]: n_iter rounds of Q <- norm(M Q), Q <- norm(M^T Q), then Q <- norm(M Q), B^T = M^T Q = Q2 R2, the SVD of
    R2^T and left = Q U^, right = Q2 V^.  -> (left [n, r], s [r], right [m, r], dropped int32 [2 n_iter + 2], info)."""
    n, m = csr[0].numel() - 1, csr_t[0].numel() - 1
    dropped = []

    def norm(Y):
        Q, R, d = psvd_orthonormalize(Y)
        dropped.append(d)
        return Q, R

    Q = omega
    for _ in range(int(n_iter)):
        Q, _ = norm(psvd_spmm(csr, m, Q))
        Q, _ = norm(psvd_spmm(csr_t, n, Q))
    Q, _ = norm(psvd_spmm(csr, m, Q))
    Q2, R2 = norm(psvd_spmm(csr_t, n, Q))
    Uh, s, Vh, info = psvd_jacobi(R2.t().contiguous(), max_sweeps)
    return psvd_gemm(Q, Uh), s, psvd_gemm(Q2, Vh), torch.cat(dropped), info


def _psvd_operands(user_vec, item_vec):
    up, ip = _f64(user_vec, "user_vec"), _f64(item_vec, "item_vec")
    U, k, I = int(user_vec.shape[0]), int(user_vec.shape[1]), int(item_vec.shape[0])
    if item_vec.shape[1] != k:
        raise ValueError(f"item_vec: expected [I, {k}], got {tuple(item_vec.shape)}")
    return (up, ip, U, I, k), U, I, user_vec.device, torch.float64, False


def psvd_rank(user_vec, item_vec, users, items=None, topk=0):
    """float64 scores [B, C] of users [B] at the candidates items [B, C] (None: every item) and, for topk > 0, the ids
    int64 [B, min(topk, C)] of the largest ones compared as float64, ties to the lower position (daisy_psvd_rank).
    -> (scores, ids or None)"""
    return _f64_rank(lib.daisy_psvd_rank, _psvd_operands(user_vec, item_vec), users, items, topk)


# ---- EASE (csrc/ease.hip; EASERecommender.py) ------------------------------------------------------------------
def _ease_square(t, name):
    p = _f64(t, name)
    n = int(t.shape[0])
    if t.shape[1] != n:
        raise ValueError(f"{name}: expected a square matrix, got {tuple(t.shape)}")
    return p, n


def ease_workspace(n, device):
    """The small workspace potrf, potri and weights share (daisy_ease_workspace_bytes): the inverses of the diagonal
    blocks, then diag(P)."""
    return _ws(lib.daisy_ease_workspace_bytes(int(n)), device)


def ease_system(G, reg):
    """A = (double) G + reg I, float64 [I, I] (daisy_ease_system); G: slim_gram's float32 matrix."""
    if not isinstance(G, torch.Tensor) or G.dim() != 2 or G.shape[0] != G.shape[1]:
        raise ValueError("G: expected a square 2-D torch.Tensor")
    n = int(G.shape[0])
    A = torch.empty(n, n, dtype=torch.float64, device=G.device)
    check(lib.daisy_ease_system(_ptr(G, torch.float32, "G"), n, float(reg), _ptr(A, torch.float64, "A"), _stream()))
    return A


def ease_potrf(A, ws=None):
    """The lower Cholesky factor of A in place (daisy_ease_potrf) -> (A, info, ws): only A's lower triangle is read and
    written; info an int32 device tensor [1]: 0, or 1 + the first column whose pivot is not positive; ws: the workspace
    ease_potri needs."""
    ap, n = _ease_square(A, "A")
    ws = ease_workspace(n, A.device) if ws is None else ws
    info = torch.zeros(1, dtype=torch.int32, device=A.device)
    check(lib.daisy_ease_potrf(ap, n, _ptr(info, torch.int32, "info"), _ptr(ws, torch.uint8, "ws"), ws.numel(), _stream()))
    return A, info, ws


def ease_potri(L, ws, inplace=False):
    """P = (L L^T)^-1 from ease_potrf's factor and workspace (daisy_ease_potri), bitwise symmetric; inplace: P takes L's
    storage.  One [n, n] scratch matrix (L^-1) lives for the duration of the call."""
    lp, n = _ease_square(L, "L")
    T = torch.empty_like(L)
    P = L if inplace else torch.empty_like(L)
    check(lib.daisy_ease_potri(lp, n, _ptr(T, torch.float64, "T"), _ptr(P, torch.float64, "P"), _ptr(ws, torch.uint8, "ws"),
                               ws.numel(), _stream()))
    return P


def ease_weights(P, ws=None, inplace=False):
    """B[i, j] = -P[i, j] / P[j, j] with a zero diagonal (daisy_ease_weights); inplace: B takes P's storage."""
    pp, n = _ease_square(P, "P")
    ws = ease_workspace(n, P.device) if ws is None else ws
    B = P if inplace else torch.empty_like(P)
    check(lib.daisy_ease_weights(pp, n, _ptr(B, torch.float64, "B"), _ptr(ws, torch.uint8, "ws"), ws.numel(), _stream()))
    return B


def ease_fit(csr, item_num, reg, offered_bytes=None):
    """EASERecommender.py:37-43 on the device -> (B float64 [I, I], info int32 [1]): slim_gram, ease_system, ease_potrf,
    ease_potri, ease_weights; the fp32 Gram matrix is freed once the system exists, the factor, the inverse and B share
    one buffer.  offered_bytes: what the fit may take (default: the device's free memory); a problem whose two fp64
    buffers do not fit is refused before anything is allocated."""
    I = int(item_num)
    dev = csr[0].device
    if offered_bytes is None:
        with torch.cuda.device(dev):
            offered_bytes = torch.cuda.mem_get_info()[0]
    check(lib.daisy_ease_fits(I, int(offered_bytes)))
    G = slim_gram(csr, I, offered_bytes=offered_bytes)
    A = ease_system(G, reg)
    del G
    A, info, ws = ease_potrf(A)
    P = ease_potri(A, ws, inplace=True)
    return ease_weights(P, ws, inplace=True), info


def _ease_operands(csr, W):
    rp, cp, vp, U = _slim_csr_ptrs(csr)
    wp, I = _ease_square(W, "W")
    return (rp, cp, vp, wp, U, I), U, I, W.device, torch.float64, False


def ease_rank(csr, W, users, items=None, topk=0):
    """float64 scores [B, C] = X[users] W at the candidates items [B, C] (None: every item) and, for topk > 0, the ids
    int64 [B, min(topk, C)] of the largest ones compared as float64, ties to the lower position (daisy_ease_rank).
    csr: slim_csr's triple of X; W float64 [I, I].  -> (scores, ids or None)"""
    return _f64_rank(lib.daisy_ease_rank, _ease_operands(csr, W), users, items, topk)


# ---- iALS (csrc/ials.hip; IALSRecommender.py) -------------------------------------------------------------------
def _ials_table(t, name):
    """(pointer, rows, row pitch, d) of an fp32 factor table: _rows' layouts, d within the kernels' limit."""
    p, ld = _rows(t, name)
    d = int(t.shape[1])
    if d < 1 or d > N.IALS_MAX_D:
        raise ValueError(f"{name}: d={d} factors outside [1, {N.IALS_MAX_D}]")
    return p, int(t.shape[0]), ld, d


def _ials_csr(csr, n_other, validate):
    """_slim_csr_ptrs plus the entry count; validate: IndexError for a column id outside [0, n_other) and ValueError for
    a row_ptr that does not rise from 0 to len(col) (one read-back)."""
    row_ptr, col, val = csr
    nnz = int(col.numel())
    if val.numel() != nnz:
        raise ValueError(f"csr: {nnz} column ids but {val.numel()} values")
    if validate:
        ok = (row_ptr[1:] >= row_ptr[:-1]).all() & (row_ptr[0] == 0) & (row_ptr[-1] == nnz)
        lo = col.min() if nnz else torch.zeros((), dtype=torch.int32, device=col.device)
        hi = col.max() if nnz else lo
        ok, lo, hi = (int(x) for x in torch.stack([ok.to(torch.int64), lo.to(torch.int64), hi.to(torch.int64)]).tolist())
        if not ok:
            raise ValueError(f"csr: row_ptr must rise from 0 to len(col) = {nnz}")
        if lo < 0 or hi >= n_other:
            raise IndexError(f"index {hi if hi >= n_other else lo} is out of bounds for the table with {n_other} rows")
    return _slim_csr_ptrs(csr) + (nnz,)


def ials_gram(Y):
    """G [d, d] = Y^T Y, float64, of a float32 table Y [n, d] whose rows may sit on a wider pitch (daisy_ials_gram):
    blocks of rows on the fp64 MFMA, their partial products added in block order; bitwise symmetric."""
    yp, n, ld, d = _ials_table(Y, "Y")
    ws = _ws(lib.daisy_ials_gram_workspace_bytes(n, d), Y.device)
    G = torch.empty(d, d, dtype=torch.float64, device=Y.device)
    check(lib.daisy_ials_gram(yp, n, ld, d, _ptr(G, torch.float64, "G"), _ptr(ws, torch.uint8, "ws"), ws.numel(), _stream()))
    return G


def ials_half_sweep(csr, Y, alpha, reg, G=None, out=None, dump=False, validate=True):
    """One half-sweep of alternating least squares (daisy_ials_half_sweep) -> (X float32 [rows, d], info int32 [1]):
    X[u] = (G + reg I + sum_i alpha r_ui y_i y_i^T)^-1 sum_i (1 + alpha r_ui) y_i over row u of csr (slim_csr's triple,
    entries in stored order), solved in fp64 by a Cholesky factorisation and rounded once.  G: ials_gram(Y), computed
    when None.  out: the table to write (rows may sit on a wider pitch).  An empty row gives zeros; info is 0, or
    1 + the smallest row whose system is not positive definite (its output is NaN).  dump=True: (X, info, A float64
    [rows, d, d], b float64 [rows, d]), the systems before factoring.  validate: IndexError for a column id outside
    [0, len(Y)) (one read-back); False trusts the ids - the kernel skips an entry whose id is out of range."""
    yp, n_other, ldy, d = _ials_table(Y, "Y")
    rp, cp, vp, rows, nnz = _ials_csr(csr, n_other, validate)
    dev = Y.device
    if G is None:
        G = ials_gram(Y)
    if G.dim() != 2 or tuple(G.shape) != (d, d):
        raise ValueError(f"G: expected [{d}, {d}], got {tuple(G.shape)}")
    if out is None:
        out = torch.empty(rows, d, dtype=torch.float32, device=dev)
    xp, xrows, ldx, xd = _ials_table(out, "out")
    if xrows != rows or xd != d:
        raise ValueError(f"out: expected [{rows}, {d}], got {tuple(out.shape)}")
    info = torch.empty(1, dtype=torch.int32, device=dev)
    A = torch.empty(rows, d, d, dtype=torch.float64, device=dev) if dump else None
    b = torch.empty(rows, d, dtype=torch.float64, device=dev) if dump else None
    check(lib.daisy_ials_half_sweep(rp, cp, vp, rows, nnz, n_other, yp, ldy, d, _ptr(G, torch.float64, "G"), float(alpha),
                                    float(reg), xp, ldx, _ptr(info, torch.int32, "info"), _ptr(A, torch.float64, "A"),
                                    _ptr(b, torch.float64, "b"), _stream()))
    return (out, info, A, b) if dump else (out, info)


def ials_objective(csr, X, Y, alpha, reg, G=None, validate=False):
    """The iALS objective (daisy_ials_objective) as a 0-dim float64 device tensor: sum over ALL cells of
    c_ui (p_ui - <x_u, y_i>)^2 with p = 1, c = 1 + alpha r on the entries of csr and p = 0, c = 1 elsewhere, plus
    reg (|X|^2 + |Y|^2) - by the Gram trick (x^T G x per row and a correction per entry), one partial per row added in
    a fixed order.  G: ials_gram(Y), computed when None."""
    yp, n_other, ldy, d = _ials_table(Y, "Y")
    xp, xrows, ldx, xd = _ials_table(X, "X")
    rp, cp, vp, rows, nnz = _ials_csr(csr, n_other, validate)
    if xrows != rows or xd != d:
        raise ValueError(f"X: expected [{rows}, {d}], got {tuple(X.shape)}")
    if G is None:
        G = ials_gram(Y)
    out = torch.empty((), dtype=torch.float64, device=Y.device)
    ws = _ws(lib.daisy_ials_objective_workspace_bytes(rows), Y.device)
    check(lib.daisy_ials_objective(rp, cp, vp, rows, nnz, n_other, xp, ldx, yp, ldy, d, _ptr(G, torch.float64, "G"),
                                   float(alpha), float(reg), C.c_void_p(out.data_ptr()), _ptr(ws, torch.uint8, "ws"),
                                   ws.numel(), _stream()))
    return out


# ---- ItemKNN / UserKNN (csrc/knn.hip; KNNCFRecommender.py) ------------------------------------------------------
KNN_SIMILARITIES = ("cosine", "pearson", "adjusted", "asymmetric", "jaccard", "tanimoto", "dice", "tversky")
_KNN_BINARY = {"jaccard": "tanimoto", "tanimoto": "tanimoto", "dice": "dice", "tversky": "tversky"}


def knn_plan(similarity, normalize):
    """(centre mode, weight mode, square-rooted norms) of a similarity name (KNNCFRecommender.py:129-151, 244-261, 313-337);
    an unknown name raises the reference's ValueError."""
    if similarity not in KNN_SIMILARITIES:
        raise ValueError("value for parameter 'similarity' not recognized. Allowed values are: 'cosine', 'pearson', "
                         "'adjusted', 'asymmetric', 'jaccard', 'tanimoto', 'dice', 'tversky'. "
                         f"Passed value was '{similarity}'")
    if similarity in _KNN_BINARY:
        return "binary", _KNN_BINARY[similarity], False
    centre = {"adjusted": "row", "pearson": "col"}.get(similarity, "none")
    if not normalize:
        return centre, "plain", True
    return centre, ("asymmetric" if similarity == "asymmetric" else "cosine"), True


def knn_row_means(csr):
    """float32 [n_rows]: the mean of every CSR row's stored values, 0 for an empty row (daisy_knn_row_means)."""
    rp, _, vp, R = _slim_csr_ptrs(csr)
    mean = torch.empty(R, dtype=torch.float32, device=csr[0].device)
    check(lib.daisy_knn_row_means(rp, vp, R, _ptr(mean, torch.float32, "mean"), _stream()))
    return mean


def knn_center(csr, n_cols, mode, mean=None):
    """A CSR with the same pattern and the values centred or set to 1 (daisy_knn_center); mode: 'none' | 'row' | 'col' |
    'binary'; mean: float32 [n_rows] ('row') or [n_cols] ('col')."""
    rp, cp, vp, R = _slim_csr_ptrs(csr)
    m = N.KNN_CENTER[mode]
    if mode in ("row", "col"):
        want = R if mode == "row" else int(n_cols)
        if mean is None or mean.numel() != want:
            raise ValueError(f"knn_center: mode '{mode}' needs {want} means")
    out = torch.empty_like(csr[2])
    if out.numel():
        check(lib.daisy_knn_center(rp, cp, vp, R, int(n_cols), m, _ptr(mean, torch.float32, "mean"),
                                   _ptr(out, torch.float32, "out"), _stream()))
    return csr[0], csr[1], out


def knn_diag(G, take_sqrt=True):
    """float32 [n]: the diagonal of G, square-rooted unless the similarity is a binary one (daisy_knn_diag)."""
    n = int(G.shape[0])
    if G.dim() != 2 or G.shape[1] != n:
        raise ValueError(f"G: expected a square matrix, got {tuple(G.shape)}")
    ss = torch.empty(n, dtype=torch.float32, device=G.device)
    check(lib.daisy_knn_diag(_ptr(G, torch.float32, "G"), n, int(bool(take_sqrt)), _ptr(ss, torch.float32, "ss"), _stream()))
    return ss


def knn_select(G, ss, mode, shrink, K, alpha=0.5):
    """The K largest weights of every column of the symmetric G float32 [n, n] (daisy_knn_select) -> (count int32 [n],
    rows int32 [n, K], vals float32 [n, K]) in slim_fit's fixed-pitch form, ascending row within a column; ties at the
    boundary go to the lower row, zeros are not kept.  mode: a key of _native.KNN_MODES."""
    n = int(G.shape[0])
    if G.dim() != 2 or G.shape[1] != n:
        raise ValueError(f"G: expected a square matrix, got {tuple(G.shape)}")
    if ss.numel() != n:
        raise ValueError(f"ss: expected {n} norms, got {ss.numel()}")
    k = int(K)
    count = torch.empty(n, dtype=torch.int32, device=G.device)
    rows = torch.empty(n, max(k, 0), dtype=torch.int32, device=G.device)
    vals = torch.empty(n, max(k, 0), dtype=torch.float32, device=G.device)
    check(lib.daisy_knn_select(_ptr(G, torch.float32, "G"), _ptr(ss, torch.float32, "ss"), n, N.KNN_MODES[mode], float(shrink),
                               float(alpha), k, _ptr(count, torch.int32, "count"), _ptr(rows, torch.int32, "rows"),
                               _ptr(vals, torch.float32, "vals"), _stream()))
    return count, rows, vals


def knn_fit(csr_D, n, similarity, shrink, K, normalize=True, csr_Dt=None, alpha=0.5, offered_bytes=None):
    """Similarity(D).compute_similarity() of KNNCFRecommender.py:235-377 on the device -> W by column (slim_columns'
    triple: w_ptr int64 [n + 1], w_row int32, w_val float32).  csr_D: the CSR of D [n_rows, n] (slim_csr); csr_Dt: the CSR
    of D^T, needed by 'pearson' alone (its column means).  Chain: centre, slim_gram, the norms, knn_select, slim_columns.
    offered_bytes: what the fit may take (default: the device's free memory); a problem whose dense G does not fit is
    refused before anything is allocated."""
    centre, mode, take_sqrt = knn_plan(similarity, normalize)
    n, k = int(n), int(K)
    dev = csr_D[0].device
    R = csr_D[0].numel() - 1
    if offered_bytes is None:
        with torch.cuda.device(dev):
            offered_bytes = torch.cuda.mem_get_info()[0]
    check(lib.daisy_knn_fits(R, n, k, int(offered_bytes)))
    mean = None
    if centre == "row":
        mean = knn_row_means(csr_D)
    elif centre == "col":
        if csr_Dt is None:
            raise ValueError("knn_fit: 'pearson' needs csr_Dt (the column means are the row means of D^T)")
        mean = knn_row_means(csr_Dt)
    D = knn_center(csr_D, n, centre, mean) if centre != "none" else csr_D
    G = slim_gram(D, n, offered_bytes=offered_bytes)
    ss = knn_diag(G, take_sqrt)
    count, rows, vals = knn_select(G, ss, mode, shrink, k, alpha)
    del G
    return slim_columns(count, rows, vals, n)


def knn_rows_of_columns(W, n):
    """The CSR (ptr int64 [n + 1], col int32 ascending, val float32) of a square matrix given by column (slim_columns'
    triple): UserKNN's left operand.  Torch ops, once per fit."""
    w_ptr, w_row, w_val = W
    nnz = int(w_ptr[-1].item())
    dev = w_ptr.device
    colid = torch.repeat_interleave(torch.arange(n, device=dev, dtype=torch.int64), w_ptr[1:] - w_ptr[:-1])
    r = w_row[:nnz].to(torch.int64)
    order = torch.argsort(r * max(n, 1) + colid)
    ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    ptr[1:] = torch.cumsum(torch.bincount(r, minlength=n), 0) if nnz else 0
    col, val = colid[order].to(torch.int32).contiguous(), w_val[:nnz][order].contiguous()
    if nnz == 0:
        col, val = col.new_zeros(1), val.new_zeros(1)
    return ptr, col, val


def _knn_operands(L, R, inner, n_cols):
    lp, lc, lv, n_rows = _slim_csr_ptrs(L)
    rp, rc, rv, nc = _slim_csr_ptrs(R)
    if nc != int(n_cols):
        raise ValueError(f"R: {nc} columns given, n_cols={n_cols}")
    return (lp, lc, lv, n_rows, int(inner), rp, rc, rv, int(n_cols)), n_rows, int(n_cols), L[0].device, torch.float64, True


def knn_rank(L, R, inner, n_cols, users, items=None, topk=0, path="auto"):
    """float64 scores [B, C] = L[users] R at the candidates items [B, C] (None: every column) and, for topk > 0, the ids
    int64 [B, min(topk, C)] of the largest ones compared as float64, ties to the lower position (daisy_knn_rank).  L: a
    CSR triple [*, inner]; R: a by-column triple [inner, n_cols].  -> (scores, ids or None)"""
    return _f64_rank(lib.daisy_knn_rank, _knn_operands(L, R, inner, n_cols), users, items, topk, path)


# ---- two-hop walk with a per-row top-K (csrc/walk2.hip; RP3betaRecommender.py) ---------------------------
def _walk2_check_sorted(csr, n_cols, name):
    """ValueError unless csr is a CSR whose columns lie in [0, n_cols), ascending and distinct within a row (one read-back)."""
    row_ptr, col, _ = csr
    nnz = int(col.numel())
    ok = (row_ptr[1:] >= row_ptr[:-1]).all() & (row_ptr[0] == 0) & (row_ptr[-1] == nnz)
    in_range = rising = torch.ones((), dtype=torch.bool, device=col.device)
    if nnz:
        c = col.to(torch.int64)
        in_range = (c.min() >= 0) & (c.max() < int(n_cols))
        first = torch.zeros(nnz + 1, dtype=torch.bool, device=col.device)
        first[row_ptr.clamp(0, nnz)] = True                        # the first entry of every row: nothing to compare with
        rising = ((c[1:] > c[:-1]) | first[1:nnz]).all()
    ok, in_range, rising = (bool(x) for x in torch.stack([ok, in_range, rising]).tolist())
    if not ok:
        raise ValueError(f"{name}: row_ptr must rise from 0 to len(col) = {nnz}")
    if not in_range:
        raise ValueError(f"{name}: a column id lies outside [0, {int(n_cols)})")
    if not rising:
        raise ValueError(f"{name}: the columns of a row must be ascending and distinct")


def walk2_topk(A, B, n_cols, K, col_scale=None, zero_diagonal=True, normalize=False, path="auto", validate=True, groups=0,
               workspace=None):
    """The K largest strictly positive entries of every row of (A B) diag(col_scale) without the dense product
    (daisy_walk2_topk) -> (count int32 [n_rows], cols int32 [n_rows, K], vals float32 [n_rows, K]) in knn_select's
    fixed-pitch form, ascending column within a row, unused slots (-1, 0).  A: a CSR triple [n_rows, inner]; B: a CSR triple
    [inner, n_cols] (slim_csr's layout, columns ascending and distinct within a row).  Row i: the products A[i, u] B[u, j]
    rounded to float32 and added in float32 over u in stored order, times col_scale[j] (float32 [n_cols]; None: no
    multiply); zero_diagonal: entry (i, i) is dropped; ties at the boundary go to the lower column; normalize: the kept
    values divided by their float32 sum.  path: 'auto' | 'lds' | 'global', bit-equal; groups: the workgroups of the launch
    (0: chosen from the shape), bit-equal for any count.  validate: ValueError unless B's columns are ascending, distinct and
    in range and A's lie in [0, inner) (one read-back each).  workspace: a uint8 device tensor to use instead of a fresh
    one."""
    if path not in N.SLIM_PATHS:
        raise ValueError(f"walk2_topk: path={path!r}: expected 'auto', 'lds' or 'global'")
    inner, nc, k = B[0].numel() - 1, int(n_cols), int(K)
    if validate:
        _walk2_check_sorted(B, nc, "B")
        _ials_csr(A, inner, True)
    ap, ac, av, n_rows = _slim_csr_ptrs(A)
    bp, bc, bv, _ = _slim_csr_ptrs(B)
    dev = A[0].device
    if col_scale is not None and col_scale.numel() != nc:
        raise ValueError(f"col_scale: expected {nc} values, got {col_scale.numel()}")
    p = N.SLIM_PATHS[path]
    count = torch.empty(n_rows, dtype=torch.int32, device=dev)
    cols = torch.empty(n_rows, max(k, 0), dtype=torch.int32, device=dev)
    vals = torch.empty(n_rows, max(k, 0), dtype=torch.float32, device=dev)
    ws = _ws(lib.daisy_walk2_workspace_bytes(n_rows, nc, p, int(groups)), dev) if workspace is None else workspace
    check(lib.daisy_walk2_topk(ap, ac, av, n_rows, inner, bp, bc, bv, nc, _ptr(col_scale, torch.float32, "col_scale"),
                               int(bool(zero_diagonal)), int(bool(normalize)), k, _ptr(count, torch.int32, "count"),
                               _ptr(cols, torch.int32, "cols"), _ptr(vals, torch.float32, "vals"), p, int(groups),
                               _ptr(ws, torch.uint8, "workspace"), ws.numel(), _stream()))
    return count, cols, vals


# ---- full ranking of many users on fp64 scores (csrc/rank_full_f64.hip) ------------------------------------
RANK_F64_TOPK_CAP = 128      # kRfTopkCap (csrc/rank_f64_users.h): the candidate buffer of a user lives in LDS


def _rank_f64_users_args(users, user_num, topk, exclude, return_scores, validate, device, score_dtype):
    """What the four *_full_rank_users share: (users int64 [n], n, topk, exclusion pointers, ids [n, topk], scores or None).
    validate: IndexError for a user id outside [0, user_num), ValueError for an exclusion that is not a CSR with ascending
    rows (ops.full_rank_users' checks, one read-back each)."""
    users = torch.as_tensor(users).to(device=device, dtype=torch.int64).reshape(-1).contiguous()
    n, topk = users.numel(), int(topk)
    if topk > RANK_F64_TOPK_CAP:
        raise ValueError(f"topk={topk} above the cap of {RANK_F64_TOPK_CAP} (the candidate buffer lives in LDS)")
    if topk < 1:
        raise ValueError(f"topk={topk} must be >= 1")
    indptr = items = None
    if exclude is not None:
        indptr, items = exclude
        if items.numel() == 0:              # (an empty tensor has no pointer to hand over)
            items = torch.zeros(1, dtype=torch.int32, device=device)
    if n and validate:
        lo, hi = (int(x) for x in torch.stack([users.min(), users.max()]).tolist())
        if lo < 0 or hi >= user_num:
            raise IndexError(f"index {hi if hi >= user_num else lo} is out of bounds for the user table with {user_num} rows")
        if exclude is not None:
            _check_exclusion(indptr, exclude[1], user_num)
    ids = torch.empty(n, topk, dtype=torch.int64, device=device)
    scores = torch.empty(n, topk, dtype=score_dtype, device=device) if return_scores else None
    excl = (_ptr(indptr, torch.int64, "exclude indptr"), _ptr(items, torch.int32, "exclude items"))
    return users, n, topk, excl, ids, scores, (indptr, items)


def _f64_full_rank_users(fn, operands, users, topk, exclude, return_scores, validate, path=None):
    """What the four *_full_rank_users share: `fn`, the family's daisy_*_full_rank_users, on its operands and the request."""
    lead, U, _, dev, score_dtype, has_path = operands
    users, n, topk, excl, ids, scores, _keep = _rank_f64_users_args(users, U, topk, exclude, return_scores, validate, dev,
                                                                    score_dtype)
    check(fn(*lead, _ptr(users, torch.int64, "users"), n, excl[0], excl[1], topk, _ptr(ids, torch.int64, "ids"),
             _ptr(scores, score_dtype, "scores"), *((N.SLIM_PATHS[path],) if has_path else ()), _stream()))
    return (ids, scores) if return_scores else ids


def ease_full_rank_users(csr, W, users, topk, exclude=None, return_scores=False, validate=True):
    """Full ranking of many users by EASE's scores X[users] W in one launch (daisy_ease_full_rank_users):
    int64 [n, topk] device ids of the best items of ALL I, best first by the float64 score of ease_rank (the same bits),
    equal scores by ascending id, NaN never selected, without the items of the user's row of `exclude` = (indptr int64
    [U + 1], items int32 ascending per row).  Positions beyond a user's eligible items hold -1 (score -inf); topk above I
    is allowed, above RANK_F64_TOPK_CAP a ValueError.  return_scores: (ids, float64 scores).  validate: as
    ops.full_rank_users.  No [n, I] array is written."""
    return _f64_full_rank_users(lib.daisy_ease_full_rank_users, _ease_operands(csr, W), users, topk, exclude, return_scores,
                                validate)


def slim_full_rank_users(csr, W, item_num, users, topk, exclude=None, return_scores=False, validate=True, path="auto"):
    """ease_full_rank_users for SLiM (daisy_slim_full_rank_users): the ranking is on slim_scores' float32 values (the
    float64 sum rounded once), returned as float32.  W: slim_columns' triple; path as slim_scores."""
    return _f64_full_rank_users(lib.daisy_slim_full_rank_users, _slim_operands(csr, W, item_num), users, topk, exclude,
                                return_scores, validate, path)


def knn_full_rank_users(L, R, inner, n_cols, users, topk, exclude=None, return_scores=False, validate=True, path="auto"):
    """ease_full_rank_users for ItemKNN / UserKNN (daisy_knn_full_rank_users): the float64 scores L[users] R of knn_rank.
    L: a CSR triple [U, inner]; R: a by-column triple [inner, n_cols]; path as knn_rank."""
    return _f64_full_rank_users(lib.daisy_knn_full_rank_users, _knn_operands(L, R, inner, n_cols), users, topk, exclude,
                                return_scores, validate, path)


def psvd_full_rank_users(user_vec, item_vec, users, topk, exclude=None, return_scores=False, validate=True):
    """ease_full_rank_users for PureSVD (daisy_psvd_full_rank_users): the float64 scores <user_vec[u], item_vec[i]> of
    psvd_rank."""
    return _f64_full_rank_users(lib.daisy_psvd_full_rank_users, _psvd_operands(user_vec, item_vec), users, topk, exclude,
                                return_scores, validate)


# ---- exact ranks of held-out items on fp64 scores (csrc/rank_positions_f64.hip) ----------------------------
RANK_COUNT_BLOCK = 512        # kRcTc (csrc/rank_count.h): targets a workgroup ranks per pass over the items (the tests' edges)


def _rank_positions_request(users, user_num, targets, exclude, validate, device):
    """The request of a *_full_rank_positions call, checked as ops.full_rank_positions checks it: -> (users int64 [n],
    pointers (exclusion indptr, exclusion items, target indptr, target items), the tensors behind the pointers)."""
    users = torch.as_tensor(users).to(device=device, dtype=torch.int64).reshape(-1).contiguous()
    n, U = users.numel(), int(user_num)
    t_indptr, t_items = targets
    indptr = items = None
    if exclude is not None:
        indptr, items = exclude
        if items.numel() == 0:              # (an empty tensor has no pointer to hand over)
            items = torch.zeros(1, dtype=torch.int32, device=device)
    if n and validate:
        lo, hi = (int(x) for x in torch.stack([users.min(), users.max()]).tolist())
        if lo < 0 or hi >= U:
            raise IndexError(f"index {hi if hi >= U else lo} is out of bounds for the user table with {U} rows")
        if exclude is not None:
            _check_exclusion(indptr, exclude[1], U)
        _check_targets(t_indptr, t_items, U)
    elif t_indptr.numel() != U + 1:
        raise ValueError(f"targets: indptr has {t_indptr.numel()} entries, the user table has {U} rows (expected {U + 1})")
    if t_items.numel() == 0:
        t_items = torch.zeros(1, dtype=torch.int32, device=device)
    ptrs = (_ptr(indptr, torch.int64, "exclude indptr"), _ptr(items, torch.int32, "exclude items"),
            _ptr(t_indptr, torch.int64, "targets indptr"), _ptr(t_items, torch.int32, "targets items"))
    return users, ptrs, (indptr, items, t_indptr, t_items)


def _rank_positions_args(users, user_num, targets, exclude, return_scores, return_eligible, validate, device, score_dtype):
    """What the *_full_rank_positions and rank_rows_positions_f32 share: _rank_positions_request and ops.full_rank_positions'
    outputs.  -> (users int64 [n], n, T, the request's pointers, out_indptr, positions, scores or None, eligible or None,
    the tensors behind the pointers)."""
    users, ptrs, keep = _rank_positions_request(users, user_num, targets, exclude, validate, device)
    n, t_indptr = users.numel(), targets[0]
    out_indptr = torch.zeros(n + 1, dtype=torch.int64, device=device)
    if n:
        torch.cumsum(t_indptr[users + 1] - t_indptr[users], 0, out=out_indptr[1:])
    T = int(out_indptr[-1]) if n else 0
    pos = torch.empty(T, dtype=torch.int32, device=device)
    scores = torch.empty(T, dtype=score_dtype, device=device) if return_scores else None
    eligible = torch.empty(n, dtype=torch.int32, device=device) if return_eligible else None
    return users, n, T, ptrs, out_indptr, pos, scores, eligible, keep


def _rank_positions_out(out_indptr, pos, scores, eligible):
    out = (out_indptr, pos)
    if scores is not None:
        out += (scores,)
    if eligible is not None:
        out += (eligible,)
    return out


def _f64_full_rank_positions(fn, operands, users, targets, exclude, return_scores, return_eligible, validate, path=None):
    """What the four *_full_rank_positions share: `fn`, the family's daisy_*_full_rank_positions, on its operands and the
    request."""
    lead, U, _, dev, score_dtype, has_path = operands
    users, n, T, ptrs, out_indptr, pos, scores, eligible, _keep = _rank_positions_args(
        users, U, targets, exclude, return_scores, return_eligible, validate, dev, score_dtype)
    check(fn(*lead, _ptr(users, torch.int64, "users"), n, *ptrs, _ptr(out_indptr, torch.int64, "out_indptr"), T,
             _ptr(pos, torch.int32, "positions"), _ptr(scores, score_dtype, "scores"), _ptr(eligible, torch.int32, "eligible"),
             *((N.SLIM_PATHS[path],) if has_path else ()), _stream()))
    return _rank_positions_out(out_indptr, pos, scores, eligible)


def ease_full_rank_positions(csr, W, users, targets, exclude=None, return_scores=False, return_eligible=False, validate=True):
    """The exact 0-based rank of every held-out item among ALL eligible items by EASE's scores X[users] W, in one launch
    (daisy_ease_full_rank_positions): for request b = users[b] and every item t of the user's row of
    `targets` = (indptr int64 [U + 1], items int32 ascending per row), the number of items outside the user's row of
    `exclude` whose float64 score is a number and comes before t's in ease_full_rank_users' order (score descending, equal
    scores by ascending id) - the index ease_full_rank_users would list t at, without its cap on topk.  -> (out_indptr int64
    [n + 1], positions int32 [T][, scores float64 [T]][, eligible int32 [n]]), ops.full_rank_positions' tuple: -1 (score
    -inf) for a target outside [0, I) or inside the exclusion row, -1 (score NaN) for a target whose score is not a number;
    eligible = the items a user can be recommended.  validate: ops.full_rank_positions' checks on users, exclude and
    targets; False skips them - the kernel then trusts the user ids and the indptr arrays, only compares the exclusion's
    contents and range-checks every target id.  No [n, I] array is written."""
    return _f64_full_rank_positions(lib.daisy_ease_full_rank_positions, _ease_operands(csr, W), users, targets, exclude,
                                    return_scores, return_eligible, validate)


def slim_full_rank_positions(csr, W, item_num, users, targets, exclude=None, return_scores=False, return_eligible=False,
                             validate=True, path="auto"):
    """ease_full_rank_positions for SLiM (daisy_slim_full_rank_positions): the ranks are on slim_scores' float32 values (the
    float64 sum rounded once), returned as float32.  W: slim_columns' triple; path as slim_scores."""
    return _f64_full_rank_positions(lib.daisy_slim_full_rank_positions, _slim_operands(csr, W, item_num), users, targets,
                                    exclude, return_scores, return_eligible, validate, path)


def knn_full_rank_positions(L, R, inner, n_cols, users, targets, exclude=None, return_scores=False, return_eligible=False,
                            validate=True, path="auto"):
    """ease_full_rank_positions for ItemKNN / UserKNN (daisy_knn_full_rank_positions): the float64 scores L[users] R of
    knn_rank.  L: a CSR triple [U, inner]; R: a by-column triple [inner, n_cols]; path as knn_rank."""
    return _f64_full_rank_positions(lib.daisy_knn_full_rank_positions, _knn_operands(L, R, inner, n_cols), users, targets,
                                    exclude, return_scores, return_eligible, validate, path)


def psvd_full_rank_positions(user_vec, item_vec, users, targets, exclude=None, return_scores=False, return_eligible=False,
                             validate=True):
    """ease_full_rank_positions for PureSVD (daisy_psvd_full_rank_positions): the float64 scores <user_vec[u], item_vec[i]>
    of psvd_rank."""
    return _f64_full_rank_positions(lib.daisy_psvd_full_rank_positions, _psvd_operands(user_vec, item_vec), users, targets,
                                    exclude, return_scores, return_eligible, validate)


# ---- masked top-k over rows of fp32 scores (csrc/rank_rows.hip) --------------------------------------------
RANK_ROWS_TOPK_CAP = 128      # kRrTopkCap (csrc/rank_rows.hip): the candidate buffer of a row lives in LDS
RANK_ROWS_STEP = 1024         # kRrStep: items a workgroup takes per step (the tests' edge sizes)


def rank_rows_f32(scores, topk, row_users=None, exclude=None, return_scores=False, validate=True, out=None):
    """The best topk items of every row of a score matrix in one launch (daisy_rank_rows_f32): scores is a
    2-D float32 device tensor with contiguous rows (its stride is the pitch: a column slice of a wider matrix is fine),
    the result int64 [m, min(topk, I)] device ids, best first - score descending, a NaN first, -0.0 equal to +0.0, equal
    scores by ascending id (ops.full_rank_users' order).  `exclude` = (indptr int64 [U + 1], items int32 ascending per
    row), the device CSR of build_user_csr, drops the items of CSR row row_users[r] (int64 [m], any order, duplicates
    allowed) from score row r; a row with fewer eligible items than topk gets -1 (score -inf) in the remaining positions.
    return_scores: (ids, float32 scores), each score the row's own stored value (the same bits).  topk above
    RANK_ROWS_TOPK_CAP raises ValueError.  validate: IndexError for a row_users entry outside [0, U), ValueError for an
    exclusion that is not such a CSR (one read-back each); False skips both - the kernel then trusts row_users and
    indptr, and only ever compares row contents.  out: (ids, scores or None) to write into instead of new tensors."""
    topk = int(topk)
    if topk > RANK_ROWS_TOPK_CAP:
        raise ValueError(f"topk={topk} above the cap of {RANK_ROWS_TOPK_CAP} (the candidate buffer lives in LDS)")
    if topk < 1:
        raise ValueError(f"topk={topk} must be >= 1")
    ptr, pitch = _rows(scores, "scores")
    m, I = int(scores.shape[0]), int(scores.shape[1])
    if m > 1 and scores.stride(0) < I:
        raise ValueError(f"scores: rows overlap (stride {scores.stride(0)} below {I} columns)")
    topk = min(topk, I)                     # as full_rank_users: argsort(...)[:topk] truncates
    if exclude is not None and row_users is None:
        raise ValueError("rank_rows_f32: an exclusion needs row_users (the CSR row of every score row)")
    indptr = items = None
    if row_users is not None:
        row_users = torch.as_tensor(row_users).to(device=scores.device, dtype=torch.int64).reshape(-1).contiguous()
        if row_users.numel() != m:
            raise ValueError(f"row_users: {row_users.numel()} entries for {m} score rows")
    if exclude is not None:
        indptr, items = exclude
        U = int(indptr.numel()) - 1
        if items.numel() == 0:              # (an empty tensor has no pointer to hand over)
            items = torch.zeros(1, dtype=torch.int32, device=scores.device)
        if m and validate:
            lo, hi = (int(x) for x in torch.stack([row_users.min(), row_users.max()]).tolist())
            if lo < 0 or hi >= U:
                raise IndexError(f"index {hi if hi >= U else lo} is out of bounds for the user table with {U} rows")
            _check_exclusion(indptr, exclude[1], U)
    if out is not None:
        ids, sc = out
    else:
        ids = torch.empty(m, topk, dtype=torch.int64, device=scores.device)
        sc = torch.empty(m, topk, dtype=torch.float32, device=scores.device) if return_scores else None
    if ids.shape != (m, topk) or (sc is not None and sc.shape != (m, topk)):
        raise ValueError(f"out: expected [{m}, {topk}] tensors")
    if m:
        check(lib.daisy_rank_rows_f32(ptr, m, I, pitch, _ptr(row_users if exclude is not None else None, torch.int64, "row_users"),
                                      _ptr(indptr, torch.int64, "exclude indptr"), _ptr(items, torch.int32, "exclude items"),
                                      topk, _ptr(ids, torch.int64, "ids"), _ptr(sc, torch.float32, "scores"), _stream()))
    return (ids, sc) if return_scores else ids


def rank_rows_positions_f32(scores, row_users, targets, exclude=None, return_scores=False, return_eligible=False,
                            validate=True, out=None):
    """The exact 0-based rank of every held-out item in its row of a score matrix, in one launch
    (daisy_rank_rows_positions_f32): scores as in rank_rows_f32; row_users int64 [m] names, for score row r,
    the row of `targets` = (indptr int64 [U + 1], items int32 ascending per row) and of `exclude` (the same form, or None).
    The position of target t is the number of items of the row outside the exclusion that come before it in rank_rows_f32's
    order - score descending, a NaN first, -0.0 equal to +0.0, equal scores by ascending id - so rank_rows_f32's ids[r,
    pos] == t wherever pos < topk, without a cap.  -> ops.full_rank_positions' tuple (out_indptr int64 [m + 1], positions
    int32 [T][, scores float32 [T]][, eligible int32 [m]]): -1 (score -inf) for a target outside [0, I) or excluded; a
    score is the row's own stored value (the same bits); eligible = I minus the distinct excluded ids in [0, I).
    validate: ops.full_rank_positions' checks on row_users, exclude and targets; False skips them.  out: (out_indptr int64
    [m + 1], positions, scores or None, eligible int32 [m] or None) to write into instead of new tensors - out_indptr
    holds the rows' offsets into positions (and scores), which may be longer than these rows' share: a caller that walks a
    large request in chunks of score rows passes slices of one out_indptr and one eligible, and the whole positions."""
    ptr, pitch = _rows(scores, "scores")
    m, I = int(scores.shape[0]), int(scores.shape[1])
    if m > 1 and scores.stride(0) < I:
        raise ValueError(f"scores: rows overlap (stride {scores.stride(0)} below {I} columns)")
    if row_users is None:
        raise ValueError("rank_rows_positions_f32: row_users is required (the CSR row of every score row)")
    dev = scores.device
    row_users = torch.as_tensor(row_users).to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    if row_users.numel() != m:
        raise ValueError(f"row_users: {row_users.numel()} entries for {m} score rows")
    U = int(targets[0].numel()) - 1
    if out is None:
        _, _, T, ptrs, out_indptr, pos, sc, eligible, _keep = _rank_positions_args(
            row_users, U, targets, exclude, return_scores, return_eligible, validate, dev, torch.float32)
    else:
        out_indptr, pos, sc, eligible = out
        if out_indptr.numel() != m + 1 or (sc is not None and sc.numel() != pos.numel()) or \
                (eligible is not None and eligible.numel() != m):
            raise ValueError(f"out: expected out_indptr [{m + 1}], scores as long as positions and eligible [{m}]")
        _, ptrs, _keep = _rank_positions_request(row_users, U, targets, exclude, validate, dev)
        T = int(pos.numel())
    if m:
        check(lib.daisy_rank_rows_positions_f32(ptr, m, I, pitch, _ptr(row_users, torch.int64, "row_users"), *ptrs,
                                                _ptr(out_indptr, torch.int64, "out_indptr"), T,
                                                _ptr(pos, torch.int32, "positions"), _ptr(sc, torch.float32, "scores"),
                                                _ptr(eligible, torch.int32, "eligible"), _stream()))
    return _rank_positions_out(out_indptr, pos, sc, eligible)


# ---- MostPop and the ranking KPIs (csrc/pop.hip, csrc/metrics.hip) ----------------------------------------
def _ids_ptr(t, name):
    """(pointer, is_i64) of a contiguous int32 / int64 device tensor of ids"""
    if isinstance(t, torch.Tensor) and t.dtype == torch.int32:
        return _ptr(t, torch.int32, name), 0
    return _ptr(t, torch.int64, name), 1


def pop_fit(items, item_num):
    """PopRecommender.py:30-33: (cnt int64 [item_num], score float64 [item_num] = cnt / (1 + cnt)) of the item column
    (int32 / int64, device)."""
    items = items.contiguous()
    ip, is64 = _ids_ptr(items, "items")
    cnt = torch.empty(int(item_num), dtype=torch.int64, device=items.device)
    score = torch.empty(int(item_num), dtype=torch.float64, device=items.device)
    check(lib.daisy_pop_fit(ip if items.numel() else None, is64, items.numel(), int(item_num), _ptr(cnt, torch.int64, "cnt"),
                            _ptr(score, torch.float64, "score"), _stream()))
    return cnt, score


def pop_rank(score, items=None, topk=1):
    """ids int64 [B, min(topk, C)] of the largest score[items[b]] (items int64 [B, C]), compared as float64, ties to the
    lower candidate position; items None: the full rank over all items, [1, topk] (daisy_pop_rank)."""
    I = score.numel()
    if items is None:
        B, Cn, gathered = 1, I, None
    else:
        items = items.to(torch.int64).contiguous()
        if items.dim() != 2:
            raise ValueError(f"items: expected [B, C], got {tuple(items.shape)}")
        B, Cn = int(items.shape[0]), int(items.shape[1])
        gathered = torch.empty(B, Cn, dtype=torch.float64, device=score.device)
    kk = min(int(topk), Cn)
    ids = torch.empty(B, max(kk, 0), dtype=torch.int64, device=score.device)
    check(lib.daisy_pop_rank(_ptr(score, torch.float64, "score"), I, _ptr(items, torch.int64, "items"), B, Cn, kk,
                             _ptr(gathered, torch.float64, "gathered"), _ptr(ids, torch.int64, "ids"), _stream()))
    return ids


def kpi_mask(metrics):
    mask = 0
    for name in metrics:
        if name not in N.KPI_IDS:
            raise ValueError(f"Invalid metric name {name}")          # metrics.py:92
        mask |= 1 << N.KPI_IDS[name]
    return mask


def ranking_kpis(pred, indptr, gt_items, users, cutoffs, metrics, item_num, disc=None, item_pop=None, cat_bits=None,
                 n_cats=0, sqrt_tab=None, per_user=False):
    """daisy_ranking_kpis: every requested KPI at every cutoff in one pass over pred (int32 / int64 [n, K], device).
    -> (names, per_user, means, cover): names = the requested per-list KPIs in slot order, per_user float64
    [len(names), nc, n] or None, means float64 [len(names), nc], cover int64 [nc] or None (the distinct ids of
    pred[:, :k])."""
    pred = pred.contiguous()
    if pred.dim() != 2:
        raise ValueError(f"pred: expected [n, K], got {tuple(pred.shape)}")
    n, K = int(pred.shape[0]), int(pred.shape[1])
    pp, is64 = _ids_ptr(pred, "pred")
    mask = kpi_mask(metrics)
    names = [m for m in sorted(N.KPI_IDS, key=N.KPI_IDS.get) if N.KPI_IDS[m] < N.KPI_PER_USER and mask >> N.KPI_IDS[m] & 1]
    cuts = (C.c_int32 * max(len(cutoffs), 1))(*[int(k) for k in cutoffs])
    nc = len(cutoffs)
    dev = pred.device
    users = users.to(torch.int64).contiguous()
    if users.numel() != n:
        raise ValueError(f"users: {users.numel()} owners for {n} lists")
    out_user = torch.empty(len(names), nc, n, dtype=torch.float64, device=dev) if (per_user and names) else None
    means = torch.empty(len(names), nc, dtype=torch.float64, device=dev)
    cover = torch.empty(nc, dtype=torch.int64, device=dev) if "coverage" in metrics else None
    ws = _ws(lib.daisy_ranking_kpis_workspace_bytes(n, nc, int(item_num), mask), dev)
    words = 0 if cat_bits is None else int(cat_bits.shape[1])
    cat_ptr = None if cat_bits is None else _ptr(cat_bits.view(torch.int64), torch.int64, "cat_bits")
    check(lib.daisy_ranking_kpis(pp, is64, n, K, _ptr(indptr, torch.int64, "indptr"), _ptr(gt_items, torch.int32, "gt_items"),
                                 indptr.numel() - 1, _ptr(users, torch.int64, "users"), cuts, nc,
                                 _ptr(disc, torch.float64, "disc"), _ptr(item_pop, torch.float64, "item_pop"), int(item_num),
                                 cat_ptr, words, int(n_cats), _ptr(sqrt_tab, torch.float64, "sqrt_tab"), mask,
                                 _ptr(out_user, torch.float64, "per_user"), _ptr(means, torch.float64, "means"),
                                 _ptr(cover, torch.int64, "cover"), _ptr(ws, torch.uint8, "ws"), ws.numel(), _stream()))
    return names, out_user, means, cover


# ---- Preprocessor and splitters (csrc/prep.hip, csrc/split.hip) -------------------------------------------
PREP_MODES = {"origin": 0, "filter": 1, "core": 2}
PREP_LEVELS = {"u": 1, "i": 2, "ui": 3}
SPLIT_METHODS = {"tloo": 0, "utfo": 1, "ufo": 2, "rloo": 3, "rsbr": 4}


def prep_encode(ids):
    """(codes int32 [n], tokens int64 [distinct]) of an int64 device column: the rank of every id among the column's
    distinct values, and those values ascending (daisy_prep_encode)."""
    ids = ids.contiguous()
    n = ids.numel()
    codes = torch.empty(n, dtype=torch.int32, device=ids.device)
    tokens = torch.empty(n, dtype=torch.int64, device=ids.device)
    distinct = C.c_int64(0)
    check(lib.daisy_prep_encode(_ptr(ids, torch.int64, "ids"), n, _ptr(codes, torch.int32, "codes"),
                                _ptr(tokens, torch.int64, "tokens"), C.byref(distinct), _stream()))
    return codes, tokens[:distinct.value]


def prep_process(users, items, rating, timestamp, threshold=None, mode="origin", level="ui", N=1, want_pop=False):
    """daisy_prep_process on int64 device columns (rating float64, None without a threshold).  -> dict: rows int64 [m]
    (positions in the input, final order), user / item int32 [m], uid_token / iid_token int64, item_pop float64
    [item_num] or None, user_num, item_num, rounds (peel rounds that removed rows)."""
    users, items, timestamp = users.contiguous(), items.contiguous(), timestamp.contiguous()
    n, dev = users.numel(), users.device
    if items.numel() != n or timestamp.numel() != n or (rating is not None and rating.numel() != n):
        raise ValueError(f"prep_process: columns of different lengths ({n} users)")
    rows = torch.empty(n, dtype=torch.int64, device=dev)
    uc, ic = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    ut, it = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2))
    pop = torch.empty(n, dtype=torch.float64, device=dev) if want_pop else None
    stats = (C.c_int64 * 4)()
    check(lib.daisy_prep_process(_ptr(users, torch.int64, "users"), _ptr(items, torch.int64, "items"),
                                 _ptr(None if rating is None else rating.contiguous(), torch.float64, "rating"),
                                 _ptr(timestamp, torch.int64, "timestamp"), n, int(threshold is not None),
                                 float(threshold) if threshold is not None else 0.0, PREP_MODES[mode], PREP_LEVELS[level],
                                 int(N), int(bool(want_pop)), _ptr(rows, torch.int64, "rows"), _ptr(uc, torch.int32, "user"),
                                 _ptr(ic, torch.int32, "item"), _ptr(ut, torch.int64, "uid_token"),
                                 _ptr(it, torch.int64, "iid_token"), _ptr(pop, torch.float64, "item_pop"), stats, _stream()))
    m, user_num, item_num, rounds = (int(x) for x in stats)
    return {"rows": rows[:m], "user": uc[:m], "item": ic[:m], "uid_token": ut[:user_num], "iid_token": it[:item_num],
            "item_pop": pop[:item_num] if want_pop else None, "user_num": user_num, "item_num": item_num, "rounds": rounds}


def split_ids(method, n, user_code=None, user_num=0, timestamp=None, size=0.5, seed=0, fold=0, device=None):
    """daisy_split_ids: (train int64, test int64) positions of a frame of n rows.  user_code int32 [n] dense codes
    (prep_encode), timestamp int64 [n] for tloo.  1 - size is formed here, on the host, as the reference forms it."""
    dev = user_code.device if user_code is not None else torch.device(device or "cuda")
    train = torch.empty(n, dtype=torch.int64, device=dev)
    test = torch.empty(n, dtype=torch.int64, device=dev)
    counts = (C.c_int64 * 2)()
    size = float(size)
    check(lib.daisy_split_ids(SPLIT_METHODS[method], _ptr(user_code, torch.int32, "user_code"),
                              _ptr(timestamp, torch.int64, "timestamp"), int(n), int(user_num), size, 1 - size,
                              int(seed) & (2 ** 64 - 1), int(fold), _ptr(train, torch.int64, "train"),
                              _ptr(test, torch.int64, "test"), counts, _stream()))
    return train[:counts[0]], test[:counts[1]]


# ---- history matrix, its CSR and first-seen order (csrc/history.hip) -------------------------------------
def _codes(t, num, name, validate):
    """an int32 device column of dense codes; validate: one device min / max against [0, num) (the kernels index with them)"""
    t = t.contiguous()
    if validate and t.numel():
        lo, hi = int(t.min()), int(t.max())
        if lo < 0 or hi >= int(num):
            raise IndexError(f"{name}: index {hi if hi >= int(num) else lo} is out of bounds for size {int(num)}")
    return t


def history_counts(row, row_num, validate=True):
    """daisy_history_counts on an int32 device column of row codes -> (history_len int64 [row_num], L, order int32 [n],
    start int64 [row_num + 1]); order / start are what history_fill reads.  L is the one word the host reads."""
    row = _codes(row, row_num, "row", validate)
    n, dev = row.numel(), row.device
    order = torch.empty(n, dtype=torch.int32, device=dev)
    start = torch.empty(int(row_num) + 1, dtype=torch.int64, device=dev)
    hlen = torch.empty(int(row_num), dtype=torch.int64, device=dev)
    longest = C.c_int64(0)
    with torch.cuda.device(dev):
        check(lib.daisy_history_counts(_ptr(row, torch.int32, "row"), n, int(row_num), _ptr(order, torch.int32, "order"),
                                       _ptr(start, torch.int64, "start"), _ptr(hlen, torch.int64, "history_len"),
                                       C.byref(longest), _stream()))
    return hlen, int(longest.value), order, start


def history_fill(order, start, col, val, row_num, L):
    """daisy_history_fill -> (history_matrix int64 [row_num, L], history_value float32 [row_num, L]); order / start from
    history_counts of the same frame, col int32 [n] (copied, never an index), val float64 [n] or None for all ones.
    Every cell is written once by the kernel: the outputs are allocated uninitialised."""
    n, dev = order.numel(), order.device
    if col.numel() != n or (val is not None and val.numel() != n):
        raise ValueError(f"history_fill: columns of different lengths ({n} rows)")
    if start.numel() != int(row_num) + 1:
        raise ValueError(f"history_fill: start has {start.numel()} entries, row_num + 1 = {int(row_num) + 1} expected")
    hid = torch.empty((int(row_num), int(L)), dtype=torch.int64, device=dev)
    hval = torch.empty((int(row_num), int(L)), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.daisy_history_fill(_ptr(order, torch.int32, "order"), _ptr(start, torch.int64, "start"),
                                     _ptr(col.contiguous(), torch.int32, "col"),
                                     _ptr(None if val is None else val.contiguous(), torch.float64, "val"), n, int(row_num),
                                     int(L), _ptr(hid, torch.int64, "history_matrix"), _ptr(hval, torch.float32, "history_value"),
                                     _stream()))
    return hid, hval


def history_csr(row, col, val, row_num, col_num, validate=True):
    """daisy_history_csr on int32 device code columns (val float64 [n] or None for all ones) -> (row_ptr int64
    [row_num + 1], col int32 [nnz], val float32 [nnz], L): byte for byte what vae_history_csr makes of the padded pair of
    the same frame, without the padded pair."""
    row, col = _codes(row, row_num, "row", validate), _codes(col, col_num, "col", validate)
    n, dev = row.numel(), row.device
    if col.numel() != n or (val is not None and val.numel() != n):
        raise ValueError(f"history_csr: columns of different lengths ({n} rows)")
    row_ptr = torch.empty(int(row_num) + 1, dtype=torch.int64, device=dev)
    out_col = torch.empty(n, dtype=torch.int32, device=dev)
    out_val = torch.empty(n, dtype=torch.float32, device=dev)
    totals = (C.c_int64 * 2)()
    with torch.cuda.device(dev):
        check(lib.daisy_history_csr(_ptr(row, torch.int32, "row"), _ptr(col, torch.int32, "col"),
                                    _ptr(None if val is None else val.contiguous(), torch.float64, "val"), n, int(row_num),
                                    int(col_num), _ptr(row_ptr, torch.int64, "row_ptr"), _ptr(out_col, torch.int32, "col"),
                                    _ptr(out_val, torch.float32, "val"), totals, _stream()))
    nnz = int(totals[0])
    return row_ptr, out_col[:nnz].clone(), out_val[:nnz].clone(), int(totals[1])


def history_first_seen(ids, id_num, validate=True):
    """daisy_history_first_seen: the distinct values of an int32 device column (< id_num) in order of first appearance,
    int64 (what pandas.unique returns)."""
    ids = _codes(ids, id_num, "ids", validate)
    n, dev = ids.numel(), ids.device
    out = torch.empty(min(n, int(id_num)), dtype=torch.int64, device=dev)
    count = C.c_int64(0)
    with torch.cuda.device(dev):
        check(lib.daisy_history_first_seen(_ptr(ids, torch.int32, "ids"), n, int(id_num), _ptr(out, torch.int64, "out"),
                                           C.byref(count), _stream()))
    return out[:count.value]
