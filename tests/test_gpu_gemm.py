"""Every kernel path of csrc/gemm.hip against the strided fp64 oracle, bit for bit (gemm_oracle.py says why integer
operands make that possible): each row of gemm_oracle.CASES runs through daisy_gemm_case, must resolve to the path it
names, and must leave its whole C buffer - the canary around the product included - equal to the oracle's."""
import numpy as np
import pytest

import gemm_oracle as G
from oracle.neumf_numpy import drop_keep

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("name,path,prods", G.CASES, ids=G.CASE_IDS)
def test_gemm_case_is_bit_exact(name, path, prods):
    import torch
    from daisyrec_amd import _native as N, ops

    def up(x, bf16):
        t = torch.from_numpy(x).cuda()
        return t.to(torch.bfloat16) if bf16 else t          # (exact: the values are bf16 numbers where bf16 is stored)

    runs, descs = [], []
    for s in prods:
        g, d = G.make_data(s, seed=G.CASE_IDS.index(name))
        h, c16 = s["launcher"] == G.LAUNCH_H, bool(s["c_bf16"])
        dev = {"A": up(d["A"], h), "B": up(d["B"], h), "C": up(d["C0"], c16)}
        if d["bias"] is not None:
            dev["bias"] = up(d["bias"], False)
        if d["gate"] is not None:
            dev["gate"] = up(d["gate"], c16)
        keep = None
        if s["drop"]:
            M, Nn = s["M"], s["N"]
            keep = ops.dropout_mask(G.DROP_SEED, s["stream"], M * Nn, G.DROP_P).cpu().numpy().astype(bool).reshape(M, Nn)
            assert np.array_equal(keep, drop_keep(G.DROP_SEED, s["stream"], np.arange(M * Nn, dtype=np.uint64), G.DROP_P).reshape(M, Nn))
        descs.append(G.fill_desc(N, s, g, {k: t.data_ptr() for k, t in dev.items()}))
        runs.append((s, g, d, dev, keep))
    word = ops.gemm_case(*descs)
    torch.cuda.synchronize()
    assert N.gemm_path(word) == path
    for which, (s, g, d, dev, keep) in enumerate(runs):
        got = dev["C"].float().cpu().numpy()
        want = G.reference(s, g, d, keep)
        bad = np.flatnonzero(_bits(got) != _bits(want))
        assert bad.size == 0, (f"{name}[{which}]: {bad.size} of {got.size} elements differ, first at {bad[:8].tolist()}: "
                               f"got {got[bad[:8]].tolist()}, want {want[bad[:8]].tolist()}")
        for k, t in dev.items():          # the inputs are as they were
            if k != "C":
                assert np.array_equal(t.float().cpu().numpy(), d[k]), k
