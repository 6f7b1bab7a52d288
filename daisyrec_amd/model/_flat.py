"""A module's parameters as views of ONE flat float32 buffer, so that a dense optimiser step is a single pass over it.

Device-agnostic (the tests run it on the CPU).  The flat order is the order of the (name, parameter) pairs given;
`transposed` names the 2-D parameters that are stored transposed behind a ``.t()`` view (VAECF's ``encoder.0.weight``:
item-major in the buffer, the reference's shape in ``state_dict()``).
"""
from __future__ import annotations

import torch


def views_of(flat, named_params, transposed=()):
    """{name: view of `flat` with the parameter's shape}, laid out like `flatten_parameters` does (the gradient tables
    of a flat gradient buffer)."""
    out, off = {}, 0
    for name, p in named_params:
        n = p.numel()
        if name in transposed:
            rows, cols = p.shape
            out[name] = flat[off:off + n].view(cols, rows).t()
        else:
            out[name] = flat[off:off + n].view(p.shape)
        off += n
    return out


def flatten_parameters(named_params, device, transposed=()):
    """Copy every parameter into one flat float32 buffer on `device` and make the parameters views of it; returns the
    buffer.  Values, shapes and ``state_dict()`` stay as they are."""
    named = list(named_params)
    flat = torch.empty(sum(p.numel() for _, p in named), dtype=torch.float32, device=device)
    views = views_of(flat, named, transposed)
    for name, p in named:
        views[name].copy_(p.data)
        p.data = views[name]
    return flat


def views_live(flat, params):
    """Is `flat` still the parameters' storage, in this order?  Anything that re-homes ``p.data`` (``model.cpu()``
    followed by ``model.cuda()``, a dtype round trip, ...) leaves every parameter on the device but none a view of
    `flat`: only the addresses tell."""
    if flat is None:
        return False
    off, base = 0, flat.data_ptr()
    for p in params:
        if p.device != flat.device or p.dtype != flat.dtype or p.data_ptr() != base + flat.element_size() * off:
            return False
        off += p.numel()
    return off == flat.numel()
