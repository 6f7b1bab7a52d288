"""The C-ABI library loads (no GPU needed) and exports exactly what include/daisyrec_amd.h
declares; the Python binding covers every declared entry point."""
import ctypes
import os
import re

from conftest import ROOT


def _declared():
    src = open(os.path.join(ROOT, "include", "daisyrec_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(daisy_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported_and_bound():
    from daisyrec_amd import _native as N
    names = _declared()
    assert len(names) >= 25
    raw = ctypes.CDLL(N.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), f"{n} declared in the header but not exported"
        assert n in N.SIGNATURES, f"{n} has no ctypes signature"
    assert sorted(N.SIGNATURES) == names
    assert N.lib.daisy_abi_version() == N.ABI_VERSION


def test_argument_errors_do_not_need_a_gpu():
    import pytest
    from daisyrec_amd import _native as N
    # NULL / out-of-range arguments are rejected before any HIP call
    rc = N.lib.daisy_bpr_ctx_create(None, 16, 64, 10, 10)
    assert rc == N.DAISY_ERR_ARG and "NULL" in N.last_error()
    h = ctypes.c_void_p()
    rc = N.lib.daisy_bpr_ctx_create(ctypes.byref(h), 16, 100000, 10, 10)
    assert rc == N.DAISY_ERR_ARG and "unsupported d" in N.last_error()
    with pytest.raises(ValueError):
        N.check(rc)
    assert N.lib.daisy_mf_rank_workspace_bytes(0, 10) == 0


def test_fit_epoch_entries_reject_a_bad_optimiser_without_a_gpu():
    """The three library-issued epoch loops share one optimiser check (csrc/dense_opt.hip): an unknown optimiser, Adam
    without its second moment and Adagrad without its state are DAISY_ERR_ARG with the entry point's own name in front,
    before the context or any HIP call is touched (the pointers here are dummies nobody reads)."""
    from daisyrec_amd import _native as N
    buf = ctypes.create_string_buffer(256)
    d = ctypes.addressof(buf)
    ref = ctypes.byref
    pn, pf, bn = N.NeumfParams(), N.NfmParams(), N.NfmBnState()
    calls = {
        "neumf": lambda opt, s0, s1: N.lib.daisy_neumf_fit_epoch(d, ref(pn), ref(pn), d, d, d, 8, 4, 0, 1e-10, 0.0, 0.0, 0.0,
                                                                 0, 0, opt, 0.01, d, d, s0, s1, 16, d, None),
        "nfm": lambda opt, s0, s1: N.lib.daisy_nfm_fit_epoch(d, ref(pf), ref(pf), ref(bn), d, d, d, 8, 4, 0, 1e-10, 0.0, 0.0,
                                                             0.0, 0, 0, 0, opt, 0.01, d, d, s0, s1, 16, d, None),
        "vae": lambda opt, s0, s1: N.lib.daisy_vae_fit_epoch(d, d, d, d, d, d, 4, d, 8, 4, d, 0.0, 0.2, 0, 0, 0, 0, 0, opt,
                                                             0.01, s0, s1, d, None),
    }
    cases = [(4, d, d, "optimizer=4 (0 sgd, 1 adam, 2 adagrad, 3 rmsprop)"),
             (-1, d, d, "optimizer=-1 (0 sgd, 1 adam, 2 adagrad, 3 rmsprop)"),
             (1, d, None, "Adam needs both moments"),
             (1, None, d, "optimizer 1 needs its state"),
             (2, None, None, "optimizer 2 needs its state"),
             (3, None, None, "optimizer 3 needs its state")]
    for name, call in calls.items():
        for opt, s0, s1, text in cases:
            rc = call(opt, s0, s1)
            assert rc == N.DAISY_ERR_ARG, (name, opt, rc)
            assert N.last_error() == f"{name}_fit_epoch: {text}", (name, opt, N.last_error())


def test_product_path_never_imports_oracle():
    """oracle/ is test infrastructure: nothing under daisyrec_amd/ may reference it."""
    pkg = os.path.join(ROOT, "daisyrec_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), os.path.join(dp, f)
                assert "bpr_mf_numpy" not in txt or f in ("common.h",), os.path.join(dp, f)


def test_torch_library_ops_are_registered_without_a_cpu_kernel():
    """north_star: "surfaced to Python through PyTorch-ROCm custom ops" - torch.ops.daisyrec.* exist with the
    documented schemas (in-place annotations on the tables) and have NO CPU kernel: host tensors fail in the
    dispatcher instead of reaching a fallback."""
    import pytest
    import torch
    import daisyrec_amd.torch_ops as t
    for name in t.OPS:
        assert hasattr(torch.ops.daisyrec, name)
    schema = str(torch.ops.daisyrec.bpr_mf_step.default._schema)
    assert "Tensor(a!) P" in schema and "Tensor(b!) Q" in schema
    with pytest.raises(NotImplementedError, match="CPU"):
        torch.ops.daisyrec.mf_predict(torch.zeros(3, 4), torch.zeros(3, 4), torch.zeros(2, dtype=torch.long),
                                      torch.zeros(2, dtype=torch.long))
