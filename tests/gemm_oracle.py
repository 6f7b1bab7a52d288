"""A strided fp64 reference of csrc/gemm.h's GemmOp and the table of cases that pins every kernel path of csrc/gemm.hip.

Why the comparison is bit-exact: every operand value is a small integer and, for every output element,
sum_k |A(m,k)| |B(n,k)| + |bias| + |C0| stays below 2^24, so every partial sum in any order - MFMA k order, split-K slice
order, fp32 atomics - is an integer that fp32 holds exactly.  The scales (gate_scale, 1 / (1 - p) with p = 0.5) are
powers of two.  Some operand entries of the bf16-input cases are +-257, which bf16 rounds to +-256: the bf16-input
kernel must return the product of the rounded operands, the fp32 kernel that of the unrounded ones.
(tests/test_oracle_gemm.py asserts these conditions for every row; tests/test_gpu_gemm.py runs the rows.)
"""
import numpy as np

STORE, BIAS_RELU, GATE, ATOMIC = 0, 1, 2, 3           # EPI_* of csrc/gemm.h
LAUNCH, LAUNCH_H, LAUNCH_PAIR = 0, 1, 2               # DAISY_GEMM_LAUNCH*
FAM_F32, FAM_BF16IN, FAM_H, FAM_PAIR = 0, 1, 2, 3     # kernel family of the path word
DROP_P, DROP_SEED = 0.5, 0x5DEECE66D1234567
CANARY = -77.0                                        # a bf16 value no product of the table's data lands on by design
EXACT_CAP = float(1 << 24)


def bf16_round(x):
    """float32 -> nearest bf16 (ties to even), as float32"""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)) << np.uint32(16)
    return r.view(np.float32).reshape(x.shape)


def operand(P, rows, K, s_row, s_k):
    """the [rows, K] matrix P(r,k) = P[r*s_row + k*s_k] of a flat buffer, fp64"""
    idx = np.arange(rows, dtype=np.int64)[:, None] * s_row + np.arange(K, dtype=np.int64)[None, :] * s_k
    return np.asarray(P, np.float64)[idx]


def n_slices(K, k_chunk):
    return (K + k_chunk - 1) // k_chunk if k_chunk < K else 1


def gemm_ref(A, B, C0, *, sam, sak, sbn, sbk, ldc, scn, M, N, K, k_chunk, slice_stride=0, epi=STORE, bias=None,
             gate=None, ldg=0, gate_scale=1.0, keep=None, drop_scale=1.0, round_inputs=False, c_bf16=False):
    """GemmOp in fp64 on flat buffers: returns a float32 copy of C0 with the product written where the kernels write it.
    Per k slice z: acc = sum over the slice's k, then the epilogue, stored at C[m*ldc + n*scn + z*slice_stride]
    (ATOMIC with slice_stride 0: added).  keep: bool [M, N] dropout mask of element m*N + n (None: no dropout).
    round_inputs: the bf16-input mode (operands rounded first).  c_bf16: bf16 output - rounded after the epilogue; the
    gate applies to the rounded value and the result is rounded again (k_gemm_h)."""
    Am, Bm = operand(A, M, K, sam, sak), operand(B, N, K, sbn, sbk)
    if round_inputs:
        Am, Bm = bf16_round(Am.astype(np.float32)).astype(np.float64), bf16_round(Bm.astype(np.float32)).astype(np.float64)
    C = np.asarray(C0, np.float64).copy()
    scn = scn or 1
    at = np.arange(M, dtype=np.int64)[:, None] * ldc + np.arange(N, dtype=np.int64)[None, :] * scn
    G = None
    if epi == GATE and gate is not None:
        G = np.asarray(gate, np.float64)[np.arange(M, dtype=np.int64)[:, None] * ldg + np.arange(N, dtype=np.int64)[None, :]] > 0

    def rnd(v):
        return bf16_round(v.astype(np.float32)).astype(np.float64) if c_bf16 else v

    def drop(v):
        return v if keep is None else np.where(keep, v * drop_scale, 0.0)

    for z in range(n_slices(K, k_chunk)):
        k0, k1 = z * k_chunk, min(K, (z + 1) * k_chunk)
        v = Am[:, k0:k1] @ Bm[:, k0:k1].T
        if epi == BIAS_RELU:
            v = np.maximum(v + np.asarray(bias, np.float64)[None, :N], 0.0)
        if c_bf16:                       # k_gemm_h: dropout, round, gate, round
            v = rnd(drop(v))
            if G is not None:
                v = rnd(np.where(G, v * gate_scale, 0.0))
        else:                            # gemm_epilogue: gate, dropout
            if G is not None:
                v = np.where(G, v * gate_scale, 0.0)
            v = drop(v)
        if epi == ATOMIC and slice_stride == 0:
            C[at] += v
        else:
            C[at + z * slice_stride] = v
    return C.astype(np.float32)


def abs_bound(A, B, C0, *, sam, sak, sbn, sbk, M, N, K, bias=None, round_inputs=False, **_):
    """max over (m, n) of sum_k |A(m,k)| |B(n,k)| + |bias(n)| + max |C0|: what every partial sum stays below"""
    Am, Bm = np.abs(operand(A, M, K, sam, sak)), np.abs(operand(B, N, K, sbn, sbk))
    if round_inputs:
        Am, Bm = bf16_round(Am.astype(np.float32)).astype(np.float64), bf16_round(Bm.astype(np.float32)).astype(np.float64)
    b = 0.0 if bias is None else np.abs(np.asarray(bias, np.float64))[None, :N]
    return float((Am @ Bm.T + b).max() + np.abs(np.asarray(C0, np.float64)).max())


# ------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------
def P(launcher, epi, M, N, K, la="k", lb="k", **kw):
    """One product of a case.  la / lb: operand contiguous along 'k' or along its 'rows'; pad_a / pad_b: elements added to
    the other stride; off_a / off_b: the operand starts that many elements into its allocation (breaks the 16-byte
    alignment); k_chunk with slices='stored' | 'atomic' (ATOMIC only); trans: the transposed store ldc = 1, scn = M + pad_c;
    gate: a gate tensor with ldg = N + ldg_pad (else NULL); drop: dropout at p = 0.5 on stream `stream`; bf16: the
    bf16-input flag (such operands carry +-257 entries); c_bf16: bf16 output of launch_gemm_h."""
    d = dict(launcher=launcher, epi=epi, M=M, N=N, K=K, la=la, lb=lb, pad_a=0, pad_b=0, off_a=0, off_b=0, k_chunk=None,
             slices=None, trans=False, pad_c=None, gate=False, ldg_pad=0, gate_scale=2.0, drop=False, stream=3, bf16=0,
             c_bf16=0)
    assert set(kw) <= set(d), set(kw) - set(d)
    d.update(kw)
    if d["k_chunk"] is None:
        d["k_chunk"] = K
    if d["pad_c"] is None:
        d["pad_c"] = 3 if d["trans"] else 8
    if launcher == LAUNCH_H and epi != ATOMIC and "c_bf16" not in kw:
        d["c_bf16"] = 1
    return d


def F32(wn, fast, drop=0, splits=1):
    return (FAM_F32, wn, fast, drop, 0, 0, splits, 0)


def BF(wn, drop=0, splits=1):
    return (FAM_BF16IN, wn, 1, drop, 0, 0, splits, 0)


def H(wn, ak, bk, drop=0, splits=1):
    return (FAM_H, wn, 0, drop, ak, bk, splits, 0)


def PAIR(wn, az, bz):
    return (FAM_PAIR, wn, 0, 0, 0, 0, az, bz)


L, LH, LP = LAUNCH, LAUNCH_H, LAUNCH_PAIR
KK, KR, RK, RR = dict(), dict(lb="rows"), dict(la="rows"), dict(la="rows", lb="rows")
G3 = dict(pad_a=3, pad_b=3)          # K = 25 / 9 / 1 or 133 / 67 rows + 3: a stride that is a multiple of 4 again

# (name, the path the row is there for, its one or two products)
CASES = [
    # ---- k_gemm<WN, STORE, FAST>: interior float4 tiles, edge tiles, k tails, unaligned operands, the four layouts
    ("f32_store_fast_w1", F32(1, 1), [P(L, STORE, 128, 64, 32)]),
    ("f32_store_fast_w2_three_k_tiles", F32(2, 1), [P(L, STORE, 256, 256, 48)]),
    ("f32_store_fast_w2_k_rows", F32(2, 1), [P(L, STORE, 128, 128, 32, **KR)]),
    ("f32_store_fast_w2_rows_k", F32(2, 1), [P(L, STORE, 128, 128, 32, **RK)]),
    ("f32_store_fast_w2_rows_rows", F32(2, 1), [P(L, STORE, 128, 128, 32, **RR)]),
    ("f32_store_edge_m_w1_k25", F32(1, 0), [P(L, STORE, 133, 64, 25, **G3)]),
    ("f32_store_edge_mn_w1_k25", F32(1, 0), [P(L, STORE, 133, 61, 25, **G3)]),
    ("f32_store_edge_w2_n67_k25", F32(2, 0), [P(L, STORE, 133, 67, 25, **G3)]),
    ("f32_store_edge_w2_n130_k25", F32(2, 0), [P(L, STORE, 133, 130, 25, **G3)]),
    ("f32_store_edge_w2_k9", F32(2, 0), [P(L, STORE, 133, 67, 9, **G3)]),
    ("f32_store_edge_w1_k1", F32(1, 0), [P(L, STORE, 130, 61, 1, **G3)]),
    ("f32_store_1_1_1", F32(1, 0), [P(L, STORE, 1, 1, 1)]),
    ("f32_store_a_off_by_one", F32(1, 0), [P(L, STORE, 128, 64, 32, off_a=1)]),
    ("f32_store_b_off_by_one", F32(2, 0), [P(L, STORE, 128, 128, 32, off_b=1)]),
    ("f32_store_row_stride_34", F32(1, 0), [P(L, STORE, 128, 64, 32, pad_a=2)]),
    ("f32_store_whole_tiles_k40_is_not_fast", F32(1, 0), [P(L, STORE, 128, 64, 40)]),
    ("f32_store_edge_k_rows", F32(2, 0), [P(L, STORE, 133, 130, 25, pad_a=3, pad_b=2, **KR)]),
    ("f32_store_edge_rows_k", F32(2, 0), [P(L, STORE, 133, 130, 25, pad_a=3, pad_b=3, **RK)]),
    ("f32_store_edge_rows_rows", F32(2, 0), [P(L, STORE, 133, 130, 25, pad_a=3, pad_b=2, **RR)]),
    ("f32_store_edge_rows_rows_unaligned_pitch", F32(2, 0), [P(L, STORE, 133, 130, 25, **RR)]),
    ("f32_store_transposed_edge", F32(2, 0), [P(L, STORE, 133, 67, 25, trans=True, **G3)]),
    ("f32_store_transposed_fast", F32(1, 1), [P(L, STORE, 128, 64, 32, trans=True)]),
    # ---- k_gemm<WN, ATOMIC, FAST>: stored slices and atomics
    ("f32_slices2_fast_w1", F32(1, 1, splits=2), [P(L, ATOMIC, 128, 64, 32, k_chunk=16, slices="stored")]),
    ("f32_slices3_fast_w2", F32(2, 1, splits=3), [P(L, ATOMIC, 128, 128, 48, k_chunk=16, slices="stored")]),
    ("f32_slices8_fast_w1", F32(1, 1, splits=8), [P(L, ATOMIC, 128, 64, 512, k_chunk=64, slices="stored")]),
    ("f32_slices5_chunk24_short_last_w2", F32(2, 0, splits=5),
     [P(L, ATOMIC, 133, 67, 100, k_chunk=24, slices="stored")]),
    ("f32_slices6_chunk18_leaves_float4_w1", F32(1, 0, splits=6), [P(L, ATOMIC, 128, 64, 96, k_chunk=18, slices="stored")]),
    ("f32_slices6_chunk18_rows_rows_w2", F32(2, 0, splits=6), [P(L, ATOMIC, 128, 128, 96, k_chunk=18, slices="stored", **RR)]),
    ("f32_slices2_transposed_fast", F32(1, 1, splits=2),
     [P(L, ATOMIC, 128, 64, 64, k_chunk=32, slices="stored", trans=True, **RR)]),
    ("f32_slices2_transposed_edge", F32(1, 0, splits=2),
     [P(L, ATOMIC, 133, 30, 50, k_chunk=32, slices="stored", trans=True, pad_a=3, pad_b=2, **RR)]),
    ("f32_atomic_one_slice_fast_w1", F32(1, 1), [P(L, ATOMIC, 128, 64, 32, slices="atomic")]),
    ("f32_atomic_three_slices_fast_w2", F32(2, 1, splits=3), [P(L, ATOMIC, 128, 128, 48, k_chunk=16, slices="atomic")]),
    ("f32_atomic_three_slices_edge_w2", F32(2, 0, splits=3), [P(L, ATOMIC, 133, 67, 75, k_chunk=25, slices="atomic", pad_a=1, pad_b=1)]),
    ("f32_atomic_one_slice_edge_w1", F32(1, 0), [P(L, ATOMIC, 133, 61, 25, slices="atomic", **G3)]),
    # ---- k_gemm<WN, BIAS_RELU, FAST, DROP>
    ("f32_bias_fast_w1", F32(1, 1), [P(L, BIAS_RELU, 128, 64, 32)]),
    ("f32_bias_fast_w2", F32(2, 1), [P(L, BIAS_RELU, 256, 128, 32)]),
    ("f32_bias_edge_w1", F32(1, 0), [P(L, BIAS_RELU, 133, 61, 25, **G3)]),
    ("f32_bias_edge_w2", F32(2, 0), [P(L, BIAS_RELU, 133, 130, 25, **G3)]),
    ("f32_bias_drop_fast_w1", F32(1, 1, drop=1), [P(L, BIAS_RELU, 256, 64, 32, drop=True)]),
    ("f32_bias_drop_fast_w2", F32(2, 1, drop=1), [P(L, BIAS_RELU, 256, 256, 32, drop=True)]),
    ("f32_bias_drop_edge_w1", F32(1, 0, drop=1), [P(L, BIAS_RELU, 133, 61, 25, drop=True, **G3)]),
    ("f32_bias_drop_edge_w2", F32(2, 0, drop=1), [P(L, BIAS_RELU, 133, 130, 25, drop=True, **G3)]),
    # ---- k_gemm<WN, GATE, FAST, DROP>
    ("f32_gate_null_fast_w1", F32(1, 1), [P(L, GATE, 128, 64, 32)]),
    ("f32_gate_fast_w2_ldg", F32(2, 1), [P(L, GATE, 256, 256, 32, gate=True, ldg_pad=4)]),
    ("f32_gate_edge_w1_ldg", F32(1, 0), [P(L, GATE, 133, 61, 25, gate=True, ldg_pad=5, **G3)]),
    ("f32_gate_edge_w2", F32(2, 0), [P(L, GATE, 133, 130, 25, gate=True, gate_scale=0.5, **G3)]),
    ("f32_gate_null_drop_fast_w1", F32(1, 1, drop=1), [P(L, GATE, 256, 64, 32, drop=True, stream=1)]),
    ("f32_gate_drop_fast_w2", F32(2, 1, drop=1), [P(L, GATE, 256, 256, 32, gate=True, drop=True)]),
    ("f32_gate_null_drop_edge_w1", F32(1, 0, drop=1), [P(L, GATE, 133, 61, 25, drop=True, stream=1, **G3)]),
    ("f32_gate_drop_edge_w2", F32(2, 0, drop=1), [P(L, GATE, 133, 130, 25, gate=True, ldg_pad=3, drop=True, **G3)]),
    # ---- k_gemm_bf16<WN, EPI, DROP>: K = 32 and 96 in the three layouts for both tile widths, +-257 operands
    ("bf16in_store_w1_k32", BF(1), [P(L, STORE, 128, 64, 32, bf16=1)]),
    ("bf16in_bias_w1_k96", BF(1), [P(L, BIAS_RELU, 128, 64, 96, bf16=1)]),
    ("bf16in_bias_drop_w1_k32_k_rows", BF(1, drop=1), [P(L, BIAS_RELU, 128, 64, 32, bf16=1, drop=True, **KR)]),
    ("bf16in_gate_w1_k96_k_rows", BF(1), [P(L, GATE, 128, 64, 96, bf16=1, gate=True, **KR)]),
    ("bf16in_gate_drop_w1_k32_rows_rows", BF(1, drop=1), [P(L, GATE, 128, 64, 32, bf16=1, drop=True, stream=1, **RR)]),
    ("bf16in_slices3_w1_k96_rows_rows", BF(1, splits=3), [P(L, ATOMIC, 128, 64, 96, bf16=1, k_chunk=32, slices="stored", **RR)]),
    ("bf16in_atomic_w2_k32", BF(2), [P(L, ATOMIC, 256, 128, 32, bf16=1, slices="atomic")]),
    ("bf16in_gate_drop_w2_k96", BF(2, drop=1), [P(L, GATE, 256, 128, 96, bf16=1, gate=True, drop=True)]),
    ("bf16in_gate_w2_k32_k_rows", BF(2), [P(L, GATE, 256, 128, 32, bf16=1, gate=True, ldg_pad=4, **KR)]),
    ("bf16in_bias_drop_w2_k96_k_rows", BF(2, drop=1), [P(L, BIAS_RELU, 256, 256, 96, bf16=1, drop=True, **KR)]),
    ("bf16in_bias_w2_k32_rows_rows", BF(2), [P(L, BIAS_RELU, 256, 128, 32, bf16=1, **RR)]),
    ("bf16in_store_w2_k96_rows_rows", BF(2), [P(L, STORE, 256, 128, 96, bf16=1, **RR)]),
    # the bf16 flag on shapes the bf16-input kernel does not take: k_gemm, and the UNROUNDED product of the +-257 data
    ("bf16in_flag_edge_stays_f32", F32(2, 0), [P(L, STORE, 133, 67, 32, bf16=1)]),
    ("bf16in_flag_k48_stays_f32", F32(1, 1), [P(L, STORE, 128, 64, 48, bf16=1)]),
    ("bf16in_flag_chunk48_stays_f32", F32(1, 1, splits=2), [P(L, ATOMIC, 128, 64, 96, bf16=1, k_chunk=48, slices="stored")]),
    # ---- k_gemm_h<WN, BIAS_RELU, DROP, AK, BK>: bf16 storage, the bf16 epilogue through LDS
    ("h_bias_w1_kk_k32", H(1, 1, 1), [P(LH, BIAS_RELU, 128, 64, 32)]),
    ("h_bias_w1_kr_k96", H(1, 1, 0), [P(LH, BIAS_RELU, 128, 64, 96, **KR)]),
    ("h_bias_w1_rr_k32", H(1, 0, 0), [P(LH, BIAS_RELU, 128, 64, 32, **RR)]),
    ("h_bias_w2_kk_forward_remap", H(2, 1, 1), [P(LH, BIAS_RELU, 1024, 256, 96)]),
    ("h_bias_w2_kr_k32", H(2, 1, 0), [P(LH, BIAS_RELU, 128, 128, 32, **KR)]),
    ("h_bias_w2_rr_k96", H(2, 0, 0), [P(LH, BIAS_RELU, 256, 256, 96, **RR)]),
    ("h_bias_w1_kk_f32_out", H(1, 1, 1), [P(LH, BIAS_RELU, 256, 64, 96, c_bf16=0)]),
    ("h_bias_drop_w1_kk_k96", H(1, 1, 1, drop=1), [P(LH, BIAS_RELU, 256, 64, 96, drop=True)]),
    ("h_bias_drop_w1_kr_k32", H(1, 1, 0, drop=1), [P(LH, BIAS_RELU, 128, 64, 32, drop=True, **KR)]),
    ("h_bias_drop_w1_rr_k96", H(1, 0, 0, drop=1), [P(LH, BIAS_RELU, 256, 64, 96, drop=True, **RR)]),
    ("h_bias_drop_w2_kk_k32", H(2, 1, 1, drop=1), [P(LH, BIAS_RELU, 256, 256, 32, drop=True)]),
    ("h_bias_drop_w2_kr_k96", H(2, 1, 0, drop=1), [P(LH, BIAS_RELU, 256, 256, 96, drop=True, **KR)]),
    ("h_bias_drop_w2_rr_k32", H(2, 0, 0, drop=1), [P(LH, BIAS_RELU, 128, 128, 32, drop=True, **RR)]),
    # ---- k_gemm_h<WN, GATE, DROP, AK, BK>: bf16 gate with ldg > N, NULL gate, fp32 output (C16 == NULL)
    ("h_gate_w1_kk_k96_ldg", H(1, 1, 1), [P(LH, GATE, 128, 64, 96, gate=True, ldg_pad=8)]),
    ("h_gate_null_w1_kr_k32", H(1, 1, 0), [P(LH, GATE, 128, 64, 32, **KR)]),
    ("h_gate_w1_rr_f32_out", H(1, 0, 0), [P(LH, GATE, 128, 64, 32, gate=True, ldg_pad=3, c_bf16=0, **RR)]),
    ("h_gate_w2_kk_n256_ldg", H(2, 1, 1), [P(LH, GATE, 128, 256, 32, gate=True, ldg_pad=8, gate_scale=0.5)]),
    ("h_gate_null_w2_kr_f32_out", H(2, 1, 0), [P(LH, GATE, 256, 128, 96, c_bf16=0, **KR)]),
    ("h_gate_null_w2_rr_k96", H(2, 0, 0), [P(LH, GATE, 128, 128, 96, **RR)]),
    ("h_gate_null_drop_w1_kk", H(1, 1, 1, drop=1), [P(LH, GATE, 256, 64, 32, drop=True, stream=1)]),
    ("h_gate_drop_w1_kr", H(1, 1, 0, drop=1), [P(LH, GATE, 128, 64, 96, gate=True, drop=True, **KR)]),
    ("h_gate_null_drop_w1_rr", H(1, 0, 0, drop=1), [P(LH, GATE, 128, 64, 32, drop=True, stream=1, **RR)]),
    ("h_gate_drop_w2_kk", H(2, 1, 1, drop=1), [P(LH, GATE, 256, 256, 32, gate=True, ldg_pad=16, drop=True)]),
    ("h_gate_drop_w2_kr_f32_out", H(2, 1, 0, drop=1), [P(LH, GATE, 256, 256, 32, gate=True, drop=True, c_bf16=0, **KR)]),
    ("h_gate_null_drop_w2_rr", H(2, 0, 0, drop=1), [P(LH, GATE, 128, 128, 96, drop=True, stream=1, **RR)]),
    # ---- k_gemm_h<WN, ATOMIC, false, AK, BK>: the split-K tile remap (8 slices), 3 and 12 slices, stored and atomics
    ("h_slices8_w1_kk_one_tile", H(1, 1, 1, splits=8), [P(LH, ATOMIC, 128, 64, 256, k_chunk=32, slices="stored")]),
    ("h_slices8_w2_kk_2x2_tiles", H(2, 1, 1, splits=8), [P(LH, ATOMIC, 256, 256, 512, k_chunk=64, slices="stored")]),
    ("h_atomic8_w1_kr_one_tile", H(1, 1, 0, splits=8), [P(LH, ATOMIC, 128, 64, 256, k_chunk=32, slices="atomic", **KR)]),
    ("h_slices2_w2_kr_short_last", H(2, 1, 0, splits=2), [P(LH, ATOMIC, 128, 128, 96, k_chunk=64, slices="stored", **KR)]),
    ("h_atomic3_w1_rr", H(1, 0, 0, splits=3), [P(LH, ATOMIC, 128, 64, 96, k_chunk=32, slices="atomic", **RR)]),
    ("h_slices12_w2_rr_2x2_tiles", H(2, 0, 0, splits=12), [P(LH, ATOMIC, 256, 256, 384, k_chunk=32, slices="stored", **RR)]),
    ("h_atomic8_w2_rr_2x2_tiles", H(2, 0, 0, splits=8), [P(LH, ATOMIC, 256, 256, 256, k_chunk=32, slices="atomic", **RR)]),
    ("h_slices8_w2_kr_2x2_tiles", H(2, 1, 0, splits=8), [P(LH, ATOMIC, 256, 256, 256, k_chunk=32, slices="stored", **KR)]),
    ("h_slices16_w1_rr_two_row_tiles", H(1, 0, 0, splits=16), [P(LH, ATOMIC, 256, 64, 512, k_chunk=32, slices="stored", **RR)]),
    ("h_slices8_w1_rr_one_tile", H(1, 0, 0, splits=8), [P(LH, ATOMIC, 128, 64, 256, k_chunk=32, slices="stored", **RR)]),
    ("h_atomic_one_slice_w2_kk", H(2, 1, 1), [P(LH, ATOMIC, 128, 128, 32, slices="atomic")]),
    # ---- k_gemm_pair<WN, STORE | ATOMIC>: different M, K, layouts and slice counts side by side
    ("pair_store_w1_tiling_and_edge", PAIR(1, 1, 1), [P(LP, STORE, 128, 64, 32), P(LP, STORE, 70, 64, 25, **G3)]),
    ("pair_store_w2_layouts", PAIR(2, 1, 1),
     [P(LP, STORE, 133, 130, 25, pad_a=3, pad_b=2, **KR), P(LP, STORE, 128, 130, 9, pad_b=2, **RR)]),
    ("pair_atomic_w1_az_gt_bz", PAIR(1, 3, 1),
     [P(LP, ATOMIC, 128, 64, 96, k_chunk=32, slices="stored", **RR), P(LP, ATOMIC, 70, 64, 40, slices="atomic")]),
    ("pair_atomic_w1_az_lt_bz", PAIR(1, 1, 4),
     [P(LP, ATOMIC, 70, 64, 25, slices="atomic", **G3), P(LP, ATOMIC, 128, 64, 64, k_chunk=16, slices="stored")]),
    ("pair_atomic_w2_layouts", PAIR(2, 3, 2),
     [P(LP, ATOMIC, 133, 130, 50, k_chunk=24, slices="stored", pad_a=2, pad_b=2, **KR),
      P(LP, ATOMIC, 128, 130, 32, k_chunk=16, slices="atomic", pad_b=3, **RK)]),
]
CASE_IDS = [c[0] for c in CASES]


def geometry(s):
    """strides, offsets and element counts of one product of a case"""
    M, N, K = s["M"], s["N"], s["K"]
    g = {}
    g["sam"], g["sak"] = (K + s["pad_a"], 1) if s["la"] == "k" else (1, M + s["pad_a"])
    g["sbn"], g["sbk"] = (K + s["pad_b"], 1) if s["lb"] == "k" else (1, N + s["pad_b"])
    g["n_A"] = (M - 1) * g["sam"] + (K - 1) * g["sak"] + 1
    g["n_B"] = (N - 1) * g["sbn"] + (K - 1) * g["sbk"] + 1
    g["splits"] = n_slices(K, s["k_chunk"])
    if s["trans"]:                       # canary: 3 elements after each column, one column after the last
        g["ldc"], g["scn"] = 1, M + s["pad_c"]
        slice_len = (N + 1) * g["scn"]
    else:                                # canary: pad_c elements after each row, two rows after the last
        g["ldc"], g["scn"] = N + s["pad_c"], 0
        slice_len = (M + 2) * g["ldc"]
    stored = s["slices"] == "stored"
    g["slice_stride"] = slice_len if stored else 0
    g["n_C"] = (g["splits"] + 1) * slice_len if stored else slice_len        # (one more slice's worth of canary)
    g["ldg"] = N + s["ldg_pad"] if s["gate"] else 0
    g["n_gate"] = (M - 1) * g["ldg"] + N if s["gate"] else 0
    g["n_bias"] = N if s["epi"] == BIAS_RELU else 0
    return g


def make_data(s, seed):
    """the buffers of one product: float32 arrays A, B (with their off_* leading elements), C0, bias, gate.  Every element
    of every allocation is filled, so a read at a wrong stride meets a number, not a zero."""
    g = geometry(s)
    rng = np.random.default_rng(seed)

    def ints(n):
        v = rng.integers(-3, 4, n).astype(np.float32)
        if s["bf16"]:                    # +-257 on one entry in sixteen: bf16 holds 256 there
            big = rng.random(n) < 1.0 / 16
            v[big] = np.where(rng.random(int(big.sum())) < 0.5, 257.0, -257.0)
        return v

    d = {"A": ints(s["off_a"] + g["n_A"]), "B": ints(s["off_b"] + g["n_B"])}
    if s["epi"] == ATOMIC and s["slices"] == "atomic":            # accumulated into: non-zero integers
        c0 = rng.integers(1, 10, g["n_C"]) * rng.choice([-1, 1], g["n_C"])
        d["C0"] = c0.astype(np.float32)
    else:
        d["C0"] = np.full(g["n_C"], CANARY, np.float32)
    d["bias"] = ((np.arange(g["n_bias"]) * 7) % 41 - 20).astype(np.float32) if g["n_bias"] else None      # differs per column
    d["gate"] = rng.choice(np.array([-2, -1, 0, 0, 1, 2], np.float32), g["n_gate"]) if s["gate"] else None
    return g, d


def reference(s, g, d, keep):
    """the expected C buffer (float32; bf16 values where the output is bf16) of one product"""
    return gemm_ref(d["A"][s["off_a"]:], d["B"][s["off_b"]:], d["C0"], sam=g["sam"], sak=g["sak"], sbn=g["sbn"], sbk=g["sbk"],
                    ldc=g["ldc"], scn=g["scn"], M=s["M"], N=s["N"], K=s["K"], k_chunk=s["k_chunk"],
                    slice_stride=g["slice_stride"], epi=s["epi"], bias=d["bias"], gate=d["gate"], ldg=g["ldg"],
                    gate_scale=s["gate_scale"], keep=keep if s["drop"] else None, drop_scale=1.0 / (1.0 - DROP_P),
                    round_inputs=rounds_inputs(s), c_bf16=bool(s["c_bf16"]))


def rounds_inputs(s):
    """the bf16-input kernel takes this product: the row's path says so (test_oracle_gemm.py checks the path by dry run)"""
    return bool(s["bf16"]) and s.get("_family") == FAM_BF16IN


def elem_sizes(s):
    """bytes per element of (A and B, C and gate)"""
    return (2 if s["launcher"] == LAUNCH_H else 4), (2 if s["c_bf16"] else 4)


def fill_desc(N, s, g, ptr, dry_run=False):
    """N.GemmDesc of one product; ptr: addresses of the allocations A, B, C, bias, gate (the operands' off_* are added here)"""
    es_ab, _ = elem_sizes(s)
    d = N.GemmDesc()
    d.launcher, d.epilogue, d.bf16, d.c_bf16 = s["launcher"], s["epi"], s["bf16"], s["c_bf16"]
    d.A, d.B, d.C = ptr["A"] + s["off_a"] * es_ab, ptr["B"] + s["off_b"] * es_ab, ptr["C"]
    d.bias = ptr.get("bias") if s["epi"] == BIAS_RELU else None
    d.gate = ptr.get("gate") if s["gate"] else None
    for k in ("sam", "sak", "sbn", "sbk", "ldc", "scn", "ldg", "slice_stride", "n_A", "n_B", "n_C", "n_bias", "n_gate"):
        setattr(d, k, g[k])
    d.M, d.N, d.K, d.k_chunk = s["M"], s["N"], s["K"], s["k_chunk"]
    d.gate_scale = s["gate_scale"]
    d.drop_p = DROP_P if s["drop"] else 0.0
    d.drop_seed, d.drop_stream = DROP_SEED, s["stream"]
    d.dry_run = int(dry_run)
    return d


FAKE = {"A": 0x10000000, "B": 0x20000000, "C": 0x30000000, "bias": 0x40000000, "gate": 0x50000000}      # 16-byte aligned


def dry_run(N, ops, prods):
    """resolve a case without a GPU: fake, aligned allocation addresses (only their alignment is looked at)"""
    descs = [fill_desc(N, s, geometry(s), FAKE, dry_run=True) for s in prods]
    return ops.gemm_case(*descs)


# a product's family decides whether its operands are rounded: taken from the row's own path
for _name, _path, _prods in CASES:
    for _s in _prods:
        _s["_family"] = _path[0]
