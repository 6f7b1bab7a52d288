"""Host side of the exact GEMM tests (no GPU): the strided oracle against plain numpy, the exactness conditions of every
row of gemm_oracle.CASES, the kernel path every row resolves to (dry runs of daisy_gemm_case) against the full set
csrc/gemm.hip can dispatch, and the argument errors of the hook."""
import itertools

import numpy as np
import pytest

import gemm_oracle as G
from oracle.neumf_numpy import drop_keep


def keep_mask(s):
    M, N = s["M"], s["N"]
    return drop_keep(G.DROP_SEED, s["stream"], np.arange(M * N, dtype=np.uint64), G.DROP_P).reshape(M, N)


def _lay(rng, rows, K, layout, pad):
    """a random integer [rows, K] matrix and its flat buffer in the layout"""
    X = rng.integers(-3, 4, (rows, K)).astype(np.float64)
    if layout == "k":
        s_row, s_k = K + pad, 1
    else:
        s_row, s_k = 1, rows + pad
    buf = np.full((rows - 1) * s_row + (K - 1) * s_k + 1, 99.0)
    buf[np.arange(rows)[:, None] * s_row + np.arange(K)[None, :] * s_k] = X
    return X, buf, s_row, s_k


@pytest.mark.parametrize("la,lb", list(itertools.product(["k", "rows"], repeat=2)))
def test_strided_oracle_equals_numpy_in_each_layout(la, lb):
    rng = np.random.default_rng(1)
    M, N, K = 13, 7, 10
    A, abuf, sam, sak = _lay(rng, M, K, la, 2)
    B, bbuf, sbn, sbk = _lay(rng, N, K, lb, 1)
    want = A @ B.T
    kw = dict(sam=sam, sak=sak, sbn=sbn, sbk=sbk, M=M, N=N, K=K)
    # plain store with a row pitch: canary where nothing is written
    ldc = N + 2
    C = G.gemm_ref(abuf, bbuf, np.full(M * ldc, G.CANARY), ldc=ldc, scn=0, k_chunk=K, **kw).reshape(M, ldc)
    assert np.array_equal(C[:, :N], want) and np.all(C[:, N:] == G.CANARY)
    # transposed store
    scn = M + 1
    Ct = G.gemm_ref(abuf, bbuf, np.full(N * scn, G.CANARY), ldc=1, scn=scn, k_chunk=K, **kw).reshape(N, scn)
    assert np.array_equal(Ct[:, :M], want.T) and np.all(Ct[:, M:] == G.CANARY)
    # stored slices: each its own k range, their sum the product; atomics: the product added to C0
    S = G.gemm_ref(abuf, bbuf, np.zeros(4 * M * N), ldc=N, scn=0, k_chunk=3, slice_stride=M * N, epi=G.ATOMIC, **kw)
    S = S.reshape(4, M, N)
    for z in range(4):
        assert np.array_equal(S[z], A[:, 3 * z:3 * z + 3] @ B[:, 3 * z:3 * z + 3].T)
    assert np.array_equal(S.sum(0), want)
    c0 = rng.integers(1, 9, M * N).astype(np.float64)
    Ca = G.gemm_ref(abuf, bbuf, c0, ldc=N, scn=0, k_chunk=3, slice_stride=0, epi=G.ATOMIC, **kw)
    assert np.array_equal(Ca.reshape(M, N), want + c0.reshape(M, N))


def test_oracle_epilogues_and_bf16_variants():
    rng = np.random.default_rng(2)
    M, N, K = 9, 6, 8
    A, B = rng.integers(-3, 4, (M, K)).astype(np.float64), rng.integers(-3, 4, (N, K)).astype(np.float64)
    A[0, 0], B[0, 0], B[1, 0] = 257.0, 3.0, -257.0
    kw = dict(sam=K, sak=1, sbn=K, sbk=1, ldc=N, scn=0, M=M, N=N, K=K, k_chunk=K)
    z = np.zeros(M * N)
    acc = A @ B.T
    bias = np.arange(N) * 5.0 - 12
    got = G.gemm_ref(A.ravel(), B.ravel(), z, epi=G.BIAS_RELU, bias=bias, **kw).reshape(M, N)
    assert np.array_equal(got, np.maximum(acc + bias, 0))
    gate = rng.integers(-1, 2, (M, N + 2)).astype(np.float64)
    keep = rng.random((M, N)) < 0.5
    got = G.gemm_ref(A.ravel(), B.ravel(), z, epi=G.GATE, gate=gate.ravel(), ldg=N + 2, gate_scale=2.0, keep=keep, drop_scale=2.0,
                     **kw).reshape(M, N)
    assert np.array_equal(got, np.where(keep, 2.0, 0.0) * np.where(gate[:, :N] > 0, 2.0, 0.0) * acc)
    # bf16-input mode: 257 -> 256 on both operands
    Ar, Br = A.copy(), B.copy()
    Ar[0, 0], Br[1, 0] = 256.0, -256.0
    got = G.gemm_ref(A.ravel(), B.ravel(), z, round_inputs=True, **kw).reshape(M, N)
    assert np.array_equal(got, Ar @ Br.T) and not np.array_equal(got, acc)
    # bf16 output: rounded after the epilogue (257 * 3 = 771 -> 772, the nearest multiple of 4)
    got = G.gemm_ref(A.ravel(), B.ravel(), z, c_bf16=True, **kw).reshape(M, N)
    assert np.array_equal(got, G.bf16_round(acc.astype(np.float32)))
    assert G.bf16_round(np.float32([771.0, 257.0, 258.0, -77.0])).tolist() == [772.0, 256.0, 258.0, -77.0]


@pytest.mark.parametrize("name,path,prods", G.CASES, ids=G.CASE_IDS)
def test_every_row_is_exact_and_exercises_its_epilogue(name, path, prods):
    for s in prods:
        g, d = G.make_data(s, seed=G.CASE_IDS.index(name))
        A, B = d["A"][s["off_a"]:], d["B"][s["off_b"]:]
        bound = G.abs_bound(A, B, d["C0"], sam=g["sam"], sak=g["sak"], sbn=g["sbn"], sbk=g["sbk"], M=s["M"], N=s["N"], K=s["K"],
                            bias=d["bias"], round_inputs=G.rounds_inputs(s))
        scale = (s["gate_scale"] if s["gate"] else 1.0) * (2.0 if s["drop"] else 1.0)
        assert bound * max(scale, 1.0) < G.EXACT_CAP, (name, bound)
        if s["launcher"] == G.LAUNCH_H:            # bf16 storage: the operands and the gate are bf16 numbers already
            for x in (d["A"], d["B"], d["gate"]):
                assert x is None or np.array_equal(G.bf16_round(x), x)
        keep = keep_mask(s) if s["drop"] else None
        want = G.reference(s, g, d, keep)
        assert np.all(np.isfinite(want))
        if s["c_bf16"]:
            assert np.array_equal(G.bf16_round(want), want)
        assert np.array_equal(want.astype(np.float64), want.astype(np.float64).round()) or s["gate_scale"] < 1
        # what the row is there for is present in its data
        Am, Bm = G.operand(A, s["M"], s["K"], g["sam"], g["sak"]), G.operand(B, s["N"], s["K"], g["sbn"], g["sbk"])
        acc = Am @ Bm.T
        if s["bf16"] and s["M"] * s["K"] >= 1024:
            assert (np.abs(Am) == 257).any() and (np.abs(Bm) == 257).any()
            accr = G.bf16_round(Am.astype(np.float32)).astype(np.float64) @ G.bf16_round(Bm.astype(np.float32)).astype(np.float64).T
            assert (acc != accr).mean() > 0.5           # rounded and unrounded products differ almost everywhere
        if s["epi"] == G.BIAS_RELU and s["M"] * s["N"] > 64:
            pre = acc + d["bias"][None, :]
            assert (pre < 0).any() and (pre > 0).any() and len(set(d["bias"].tolist())) >= min(s["N"], 41)
        if s["gate"]:
            assert (d["gate"] > 0).any() and (d["gate"] < 0).any() and (d["gate"] == 0).any()
        if s["drop"]:
            assert 0.3 < keep.mean() < 0.7 and len({r.tobytes() for r in keep}) == s["M"]
        if s["epi"] == G.ATOMIC and s["slices"] == "atomic":
            assert np.all(d["C0"] != 0)


def _variant(epi, drop):
    return {G.STORE: "STORE", G.BIAS_RELU: "BIAS_RELU", G.GATE: "GATE", G.ATOMIC: "ATOMIC"}[epi] + ("+drop" if drop else "")


SIX = ["STORE", "BIAS_RELU", "BIAS_RELU+drop", "GATE", "GATE+drop", "ATOMIC"]
# every kernel instantiation the three launchers of csrc/gemm.hip can dispatch
DISPATCHABLE = (
    {("k_gemm", wn, fast, v) for wn in (1, 2) for fast in (0, 1) for v in SIX}
    | {("k_gemm_bf16", wn, v) for wn in (1, 2) for v in SIX}
    | {("k_gemm_h", wn, lay, v) for wn in (1, 2) for lay in ((1, 1), (1, 0), (0, 0)) for v in SIX[1:]}
    | {("k_gemm_pair", wn, v) for wn in (1, 2) for v in ("STORE", "ATOMIC")})
# combinations no caller can reach by construction, with the reason (none: every launcher takes its epilogue, tile
# width, layout and dropout from the op alone, and daisy_gemm_case reaches every launcher)
EXCLUDED = {}


def test_rows_resolve_to_the_paths_they_name_and_cover_every_dispatchable_kernel():
    from daisyrec_amd import _native as N, ops
    assert len(DISPATCHABLE) == 24 + 12 + 30 + 4
    seen = set()
    for name, path, prods in G.CASES:
        got = N.gemm_path(G.dry_run(N, ops, prods))
        assert got == path, (name, got, path)
        fam, wn, fast, drop, ak, bk, _, _ = got
        epi = prods[0]["epi"]
        if fam == G.FAM_F32:
            seen.add(("k_gemm", wn, fast, _variant(epi, drop)))
        elif fam == G.FAM_BF16IN:
            assert fast == 1
            seen.add(("k_gemm_bf16", wn, _variant(epi, drop)))
        elif fam == G.FAM_H:
            seen.add(("k_gemm_h", wn, (ak, bk), _variant(epi, drop)))
        else:
            seen.add(("k_gemm_pair", wn, _variant(epi, 0)))
    assert not (set(EXCLUDED) - DISPATCHABLE)
    assert seen - DISPATCHABLE == set()
    missing = DISPATCHABLE - seen - set(EXCLUDED)
    assert not missing, sorted(missing, key=str)
    assert not (seen & set(EXCLUDED)), "an excluded path is reachable after all"


def test_path_rule_edges_by_dry_run():
    """the eligibility rules at their thresholds: alignment, K % 16, K % 32, k_chunk % 4 / 16 / 32"""
    from daisyrec_amd import _native as N, ops

    def path(**kw):
        return N.gemm_path(G.dry_run(N, ops, [G.P(G.LAUNCH, kw.pop("epi", G.STORE), 128, 64, kw.pop("K", 64), **kw)]))

    assert path()[:3] == (G.FAM_F32, 1, 1)
    assert path(bf16=1)[:3] == (G.FAM_BF16IN, 1, 1)
    assert path(K=72)[:3] == (G.FAM_F32, 1, 0)                              # K % 16 != 0
    assert path(K=80, bf16=1)[:3] == (G.FAM_F32, 1, 1)                      # K % 32 != 0: fp32 kernel, still FAST
    assert path(off_a=4)[2] == 1 and path(off_a=2)[2] == 0 and path(off_b=3)[2] == 0
    assert path(pad_a=4)[2] == 1 and path(pad_a=6)[2] == 0
    sl = dict(epi=G.ATOMIC, slices="stored")
    assert path(k_chunk=16, bf16=1, **sl) == (G.FAM_F32, 1, 1, 0, 0, 0, 4, 0)
    assert path(k_chunk=32, bf16=1, **sl) == (G.FAM_BF16IN, 1, 1, 0, 0, 0, 2, 0)
    assert path(k_chunk=20, **sl)[2] == 0 and path(k_chunk=18, **sl)[2] == 0
    assert path(k_chunk=64, **sl)[6] == 1 and path(k_chunk=63, **sl)[6] == 2


def _err(N, ops, descs, text):
    with pytest.raises(ValueError) as e:
        ops.gemm_case(*descs)
    assert text in str(e.value), (text, str(e.value))


def test_argument_errors_stop_before_hip():
    from daisyrec_amd import _native as N, ops

    def desc(s):
        return G.fill_desc(N, s, G.geometry(s), G.FAKE, dry_run=True)

    # each buffer one element too short names its field; the exact count passes
    bias_s = G.P(G.LAUNCH, G.BIAS_RELU, 133, 61, 25, **G.G3)
    gate_s = G.P(G.LAUNCH, G.GATE, 133, 130, 25, gate=True, ldg_pad=3, **G.G3)
    slice_s = G.P(G.LAUNCH, G.ATOMIC, 133, 67, 100, k_chunk=24, slices="stored", trans=True)
    h_s = G.P(G.LAUNCH_H, G.GATE, 128, 64, 32, gate=True, ldg_pad=8)
    for s, fields in ((bias_s, ("n_A", "n_B", "n_bias")), (gate_s, ("n_A", "n_B", "n_gate")), (h_s, ("n_A", "n_B", "n_gate"))):
        ops.gemm_case(desc(s))
        for f in fields:
            d = desc(s)
            setattr(d, f, getattr(d, f) - 1)
            _err(N, ops, [d], f)
    for s in (bias_s, gate_s, slice_s, h_s):          # n_C: the last element of the last slice
        g = G.geometry(s)
        last = (s["M"] - 1) * g["ldc"] + (s["N"] - 1) * (g["scn"] or 1) + (g["splits"] - 1) * g["slice_stride"]
        d = desc(s)
        d.n_C = last + 1
        ops.gemm_case(d)
        d.n_C = last
        _err(N, ops, [d], "n_C")
    pa, pb = G.P(G.LAUNCH_PAIR, G.STORE, 128, 64, 32), G.P(G.LAUNCH_PAIR, G.STORE, 70, 64, 25)
    ops.gemm_case(desc(pa), desc(pb))
    d = desc(pb)
    d.n_B -= 1
    _err(N, ops, [desc(pa), d], "b.n_B")
    # NULL pointers, non-positive sizes
    for f in ("A", "B", "C", "bias"):
        d = desc(bias_s)
        setattr(d, f, None)
        _err(N, ops, [d], "NULL")
    for f in ("M", "N", "K", "k_chunk"):
        for v in (0, -1):
            d = desc(bias_s)
            setattr(d, f, v)
            _err(N, ops, [d], "positive")
    for f in ("sam", "sak", "sbn", "sbk", "ldc"):
        d = desc(bias_s)
        setattr(d, f, 0)
        _err(N, ops, [d], f)
    # launcher / epilogue pairs that gemm.hip does not instantiate
    for launcher, epi in ((G.LAUNCH_H, G.STORE), (G.LAUNCH_PAIR, G.BIAS_RELU), (G.LAUNCH_PAIR, G.GATE), (G.LAUNCH, 4), (3, G.STORE)):
        d = desc(G.P(G.LAUNCH, G.STORE, 128, 64, 32))
        d.launcher, d.epilogue = launcher, epi
        descs = [d, desc(pb)] if launcher == G.LAUNCH_PAIR else [d]
        if launcher == G.LAUNCH_PAIR:
            descs[1].epilogue = epi
        _err(N, ops, descs, "launcher")
    _err(N, ops, [desc(pa)], "two descriptors")
    _err(N, ops, [desc(bias_s), desc(pb)], "two descriptors")
    # a pair of different N; split-K or slices under a storing epilogue; dropout under one that has none
    _err(N, ops, [desc(pa), desc(G.P(G.LAUNCH_PAIR, G.STORE, 70, 60, 25))], "a.N == b.N")
    d = desc(G.P(G.LAUNCH, G.STORE, 128, 64, 32))
    d.k_chunk = 16
    _err(N, ops, [d], "k_chunk")
    d = desc(G.P(G.LAUNCH, G.STORE, 128, 64, 32))
    d.slice_stride = 128 * 72
    _err(N, ops, [d], "slice_stride")
    d = desc(G.P(G.LAUNCH, G.STORE, 128, 64, 32))
    d.drop_p = 0.5
    _err(N, ops, [d], "drop_p")
    # launch_gemm_h: a partial tile, K % 32 != 0, a misaligned operand, the (A rows, B k) layout, unaligned bf16 output rows
    ok = G.P(G.LAUNCH_H, G.BIAS_RELU, 128, 64, 32)
    ops.gemm_case(desc(ok))
    for bad in (G.P(G.LAUNCH_H, G.BIAS_RELU, 130, 64, 32), G.P(G.LAUNCH_H, G.BIAS_RELU, 128, 60, 32),
                G.P(G.LAUNCH_H, G.BIAS_RELU, 128, 192, 32), G.P(G.LAUNCH_H, G.BIAS_RELU, 128, 64, 48),
                G.P(G.LAUNCH_H, G.BIAS_RELU, 128, 64, 32, off_a=1), G.P(G.LAUNCH_H, G.BIAS_RELU, 128, 64, 32, off_b=4),
                G.P(G.LAUNCH_H, G.BIAS_RELU, 128, 64, 32, pad_a=4), G.P(G.LAUNCH_H, G.BIAS_RELU, 128, 64, 32, la="rows"),
                G.P(G.LAUNCH_H, G.ATOMIC, 128, 64, 96, k_chunk=48, slices="stored")):
        _err(N, ops, [desc(bad)], "launch_gemm_h needs")
    _err(N, ops, [desc(G.P(G.LAUNCH_H, G.BIAS_RELU, 128, 64, 32, pad_c=4))], "ldc")
    _err(N, ops, [desc(G.P(G.LAUNCH_H, G.GATE, 128, 64, 32, gate=True, ldg_pad=4))], "ldg")
    _err(N, ops, [desc(G.P(G.LAUNCH_H, G.GATE, 128, 64, 32, trans=True))], "scn")
    d = desc(G.P(G.LAUNCH, G.STORE, 128, 64, 32))
    d.c_bf16 = 1
    _err(N, ops, [d], "c_bf16")
