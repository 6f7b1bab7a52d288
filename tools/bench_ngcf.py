#!/usr/bin/env python
"""NGCF training throughput on one MI355X, on tools/bench_lightgcn.py's Amazon-Book-shaped synthetic graph
(52 643 users x 91 599 items, 2.38 M interactions); factors 64, hidden [64, 64, 64], B = 4 096 and 256.

Reported (one JSON line each):
  copy       the device-copy rate of this process (the yardstick of the byte fractions)
  layer_fwd  daisy_ngcf_layer_forward alone: algorithmic bytes N (2 d_in + d_out + 1) * 4 over kernel time
  layer_bwd  daisy_ngcf_layer_backward + daisy_ngcf_wgrad_reduce: algorithmic bytes N (6 d_in + 2 d_out + 1) * 4
             (reads dY, Y, norm, E, X, the concat gradient; writes dE, dX) over their time
  spmm       daisy_lgcn_spmm_ex on a 64-wide slice of the concat buffer (forward form and masked transpose)
  step       ms per NGCF step (full propagation + loss + backward + Adam), median of three timed regions of --steps
             steps after warm-up; the LightGCN L = 3 step at the same shapes; the stock-torch restatement of the
             reference's formulation (autograd + torch.sparse.mm + torch.optim.Adam) on the same GPU

    python tools/bench_ngcf.py [--steps 50] [--no-torch] > profiles/rNN_bench_ngcf.txt
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np
import scipy.sparse as sp
import torch
import torch.nn as nn
import torch.nn.functional as F

from bench_lightgcn import I, NNZ, U, synth
from daisyrec_amd import ops
from daisyrec_amd.model.LightGCNRecommender import LightGCN
from daisyrec_amd.model.NGCFRecommender import NGCF

FACTORS, HIDDEN = 64, [64, 64, 64]
dev = torch.device("cuda", 0)


def ev():
    return torch.cuda.Event(enable_timing=True)


def timed(fn, reps, regions=3, warm=3):
    """median over `regions` timed regions of `reps` calls (ms per call)"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(regions):
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return statistics.median(out)


def emit(**kw):
    print(json.dumps(kw), flush=True)


class TorchNGCF(nn.Module):
    """The reference's NGCF formulation (NGCFRecommender.py:38-209, BPR, no dropout) in stock torch on the device:
    autograd through torch.sparse.mm, nn.Linear, F.leaky_relu and F.normalize; torch.optim.Adam."""

    def __init__(self, adj, widths):
        super().__init__()
        self.adj = adj
        self.embed_user = nn.Embedding(U, widths[0])
        self.embed_item = nn.Embedding(I, widths[0])
        self.lin = nn.ModuleList(nn.Linear(a, b) for a, b in zip(widths[:-1], widths[1:]))
        self.inter = nn.ModuleList(nn.Linear(a, b) for a, b in zip(widths[:-1], widths[1:]))

    def step(self, opt, u, i, j):
        E = torch.cat([self.embed_user.weight, self.embed_item.weight], 0)
        outs = [E]
        for lin, inter in zip(self.lin, self.inter):
            X = torch.sparse.mm(self.adj, E)
            E = F.normalize(F.leaky_relu(lin(E + X) + inter(X * E), 0.2), p=2, dim=1)
            outs.append(E)
        out = torch.cat(outs, 1)
        ue, pe, ne = out[u], out[U + i], out[U + j]
        loss = -(1e-10 + torch.sigmoid((ue * pe).sum(1) - (ue * ne).sum(1))).log().sum()
        opt.zero_grad()
        loss.backward()
        opt.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-lightgcn", action="store_true")
    args = ap.parse_args()
    gu, gi = synth()
    import logging
    base = dict(gpu="0", logger=logging.getLogger("b"), epochs=1, lr=0.01, topk=50, user_num=U, item_num=I,
                inter_matrix=sp.coo_matrix((np.ones(NNZ, np.float32), (gu, gi)), shape=(U, I)), factors=FACTORS,
                reg_1=0.0, reg_2=0.0, loss_type="BPR", optimizer="default", init_method="default", early_stop=False,
                progress=False, seed=2022)
    N = U + I
    # ---- yardstick: device copy in this process
    a = torch.empty(256 << 20, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    ms = timed(lambda: b.copy_(a), 20)
    copy_gbps = 2 * a.numel() * 4 / ms / 1e6
    emit(copy={"ms": ms, "GBps": copy_gbps, "bytes": 2 * a.numel() * 4})
    del a, b
    torch.manual_seed(0)
    model = NGCF(dict(base, hidden_size_list=HIDDEN, node_dropout=0.0, mess_dropout=0.0))
    model._params()
    graph = model._adj()
    w = model._widths
    D = sum(w)
    emit(graph={"nodes": N, "entries": graph.nnz}, widths=w)
    # ---- the layer kernels alone (64 -> 64)
    din, dout = 64, 64
    cat = torch.randn(N, D, device=dev)
    E, Y = cat[:, :din], cat[:, din:din + dout]
    X = torch.randn(N, din, device=dev)
    norm = torch.empty(N, device=dev)
    W1, W2 = torch.randn(dout, din, device=dev) * 0.1, torch.randn(dout, din, device=dev) * 0.1
    b1, b2 = torch.zeros(dout, device=dev), torch.zeros(dout, device=dev)
    fwd = lambda: ops.ngcf_layer_forward(E, X, W1, b1, W2, b2, Y, norm, 0.1, 1, 0)  # noqa: E731
    ms = timed(fwd, 50)
    alg = N * (2 * din + dout + 1) * 4
    emit(layer_fwd={"ms": ms, "algorithmic_MB": alg / 1e6, "GBps": alg / ms / 1e6, "frac_of_copy": alg / ms / 1e6 / copy_gbps})
    G = torch.randn(N, D, device=dev)
    dY = G[:, din:din + dout]
    dE, dX = torch.empty(N, din, device=dev), torch.empty(N, din, device=dev)
    ws = torch.empty(ops.ngcf_ws_bytes(N, din, dout), dtype=torch.uint8, device=dev)
    gw = [torch.zeros_like(t) for t in (W1, b1, W2, b2)]

    def bwd():
        ops.ngcf_layer_backward(dY, Y, norm, E, X, W1, W2, dE, dX, ws, 0.1, 1, 0, gprev=G[:, :din])
        ops.ngcf_wgrad_reduce(ws, N, din, dout, *gw)
    ms = timed(bwd, 50)
    alg = N * (6 * din + 2 * dout + 1) * 4
    emit(layer_bwd={"ms": ms, "algorithmic_MB": alg / 1e6, "GBps": alg / ms / 1e6, "frac_of_copy": alg / ms / 1e6 / copy_gbps,
                    "workspace_MB": ws.numel() / 1e6})
    # ---- the sparse products on a slice of the concat buffer
    out = torch.empty(N, din, device=dev)
    ms_f = timed(lambda: graph.spmm_ex(E, out=out), 20)
    ms_t = timed(lambda: graph.spmm_ex(out, out=dE, accumulate=True, keep=(0.1, 5), transpose=True), 20)
    alg = graph.nnz * (4 * din + 20) + N * 4 * din
    emit(spmm={"forward_ms": ms_f, "masked_transpose_accumulate_ms": ms_t, "algorithmic_MB": alg / 1e6,
               "GBps": alg / ms_f / 1e6, "frac_of_copy": alg / ms_f / 1e6 / copy_gbps})
    # ---- training steps
    loss_id = ops.loss_id("BPR")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    flat = model._params()
    lg = None
    if not args.no_lightgcn:
        torch.manual_seed(0)
        lg = LightGCN(dict(base, num_layers=3))
        LE0 = lg._ego()
        lg._adj()
        lout, LG_, ldE0 = torch.empty_like(LE0), torch.empty_like(LE0), torch.zeros_like(LE0)
    res = {}
    for B in (4096, 256):
        u = torch.randint(0, U, (B,), device=dev, generator=g, dtype=torch.int32)
        i = torch.randint(0, I, (B,), device=dev, generator=g, dtype=torch.int32)
        j = torch.randint(0, I, (B,), device=dev, generator=g, dtype=torch.int32)
        ctx, ctx_ego = model._contexts(B, loss_id)
        optim = ops.DenseOptimizer("adam", 0.01)

        def step():
            model._batch_grads(ctx, ctx_ego, u, i, j, loss_id)
            optim.next_step()
            optim.step(flat, model._gflat)
        ng_ms = timed(step, args.steps)
        row = {"B": B, "ngcf_ms_per_step": ng_ms, "samples_per_s": B / ng_ms * 1e3}
        ctx.close()
        ctx_ego.close()
        if lg is not None:
            lctx = ops.BprContext(B, FACTORS, U, I)
            lopt = ops.DenseOptimizer("adam", 0.01)

            def lstep():
                lg._batch_grads(lctx, LE0, lout, LG_, ldE0, u, i, j, loss_id)
                lopt.next_step()
                lopt.step(lg._flat, ldE0.view(-1))
            lg_ms = timed(lstep, args.steps)
            lctx.close()
            row.update(lightgcn_L3_ms_per_step=lg_ms, ngcf_over_lightgcn=ng_ms / lg_ms)
        res[B] = row
        emit(step=row)
    if not args.no_torch:
        row, col, val = graph.coo()
        adj = torch.sparse_coo_tensor(torch.stack([row.long(), col.long()]), val, (N, N)).coalesce()
        torch.manual_seed(0)
        tm = TorchNGCF(adj, w).to(dev)
        topt = torch.optim.Adam(tm.parameters(), lr=0.01)
        for B in (4096, 256):
            u = torch.randint(0, U, (B,), device=dev, generator=g)
            i = torch.randint(0, I, (B,), device=dev, generator=g)
            j = torch.randint(0, I, (B,), device=dev, generator=g)
            t_ms = timed(lambda: tm.step(topt, u, i, j), args.steps)
            emit(torch_reference_formulation={"B": B, "ms_per_step": t_ms,
                                              "ngcf_speedup": t_ms / res[B]["ngcf_ms_per_step"]})


if __name__ == "__main__":
    main()
