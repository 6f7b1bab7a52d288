// The MFMA products on gfx950 behind NeuMF's tower, Multi-VAE's layers and the daisy_gemm_* entry points:
//   k_gemm<WN, EPI, FAST, DROP>      fp32 MFMA 32x32x2 tiles, LDS-staged, register-prefetched (k_gemm_pair: two in one launch)
//   k_gemm_bf16<WN, EPI, DROP>       fp32 storage, operands rounded to bf16 on their way to LDS (32x32x16 MFMA)
//   k_gemm_h<WN, EPI, DROP, AK, BK>  bf16 storage
// Epilogues (EPI_*, gemm.h): store, bias + ReLU, gate, split-K partial products; the middle two with dropout.
#include "gemm.h"
#include "mfma.h"

#include <type_traits>

#ifndef DAISY_BKH
#define DAISY_BKH 32        // k depth of the bf16-storage GEMM's tiles (32 or 64; -DDAISY_BKH=64 to try the other)
#endif

namespace daisy {

constexpr int kBK = 16;        // k depth of an LDS tile
constexpr int kLdsPad = 4;

template <int WN, int EPI, bool FAST, bool DROP>
__device__ __forceinline__ void gemm_epilogue(const GemmOp &op, floatx16 (&acc)[2][WN], int64_t m0, int n0, int wm,
                                              int wn, int lane, unsigned zslice) {
    // lane holds column (lane % 32), rows (i/4)*8 + (lane/32)*4 + i%4 of each 32x32 block (all MFMA
    // 32x32 shapes share this C/D map on gfx950).  epilogue: lane holds column (lane % 32), rows (i/4)*8 + (lane/32)*4 + i%4 of each 32x32 block.
    // 32-bit offsets from the tile origin (a tile spans < 2^31 elements of C: 128 rows x ldc)
    const int scn = op.scn ? (int)op.scn : 1;
    float *__restrict__ Ct = op.C + m0 * op.ldc + (int64_t)n0 * scn;
    // (the k slice this workgroup computed - k_gemm_h remaps workgroups to tiles, so that is NOT blockIdx.z there: until round 6
    // the slices of the bf16-storage weight gradients landed in the slot of blockIdx.z, two workgroups per slot whenever the
    // slice count was a multiple of 8 and an output had fewer than 8 tiles - partial products lost, unseen by tests that
    // allowed 25 %; found by the bf16 oracle at 2 %)
    if constexpr (EPI == EPI_ATOMIC) Ct += (int64_t)zslice * op.slice_stride;
    const float *__restrict__ Gt = (EPI == EPI_GATE && op.gate) ? op.gate + m0 * op.ldg + n0 : nullptr;
    const int ldc = (int)op.ldc, ldg = (int)op.ldg;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < WN; ++ni) {
            const int nl = wn * 32 * WN + ni * 32 + lane % 32;
            float bias = 0.f;
            if constexpr (EPI == EPI_BIAS_RELU) bias = (FAST || n0 + nl < op.N) ? op.bias[n0 + nl] : 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int ml = wm * 64 + mi * 32 + (i / 4) * 8 + (lane / 32) * 4 + (i % 4);
                if (!FAST && (m0 + ml >= op.M || n0 + nl >= op.N)) continue;
                float v = acc[mi][ni][i];
                if constexpr (EPI == EPI_BIAS_RELU) v = fmaxf(v + bias, 0.f);
                if constexpr (EPI == EPI_GATE)
                    if (Gt) v = (Gt[ml * ldg + nl] > 0.f) ? v * op.gate_scale : 0.f;
                if constexpr (DROP)
                    if (op.drop_thresh)
                        v = drop_keep(op.drop_seed, op.drop_stream,
                                      (uint64_t)(m0 + ml) * (uint64_t)op.N + (uint64_t)(n0 + nl), op.drop_thresh)
                                ? v * op.drop_scale : 0.f;
                if constexpr (EPI == EPI_ATOMIC) {
                    if (op.slice_stride) Ct[ml * ldc + nl * scn] = v;
                    else unsafeAtomicAdd(Ct + ml * ldc + nl * scn, v);
                } else Ct[ml * ldc + nl * scn] = v;
            }
        }
}

// C = A * B^T-style contraction over k with arbitrary strides.  WN: 32-column MFMA blocks per wave
// (block tile = 128 x 64*WN).  Operand tiles go global -> registers -> LDS (k-major, so the MFMA
// fragment reads are conflict free; two LDS stages, one barrier per k tile) with the next tile's
// loads in flight during the MFMAs.  Interior tiles of 16-byte aligned operands take a branch-free
// float4 path (a guarded load costs a branch and a vmcnt drain each); edge tiles, k tails and
// unaligned operands take the guarded scalar path.
// FAST: every tile is interior, both operands qualify for the float4 path and the k range is a multiple
// of kBK (checked by launch_gemm) - the guarded loader and its address registers are compiled out, which
// is what lets four waves per SIMD share the MFMA pipe.
template <int WN, int EPI, bool FAST, bool DROP>
__device__ __forceinline__ void gemm_f32_tile(const GemmOp &op, unsigned bx, unsigned by, unsigned bz) {
    constexpr int BM = kGemmBM, BN = 64 * WN;
    constexpr int EA = BM * kBK / kBlock, EB = BN * kBK / kBlock;     // elements per thread per tile
    constexpr int LA = BM + kLdsPad, LB = BN + kLdsPad;
    __shared__ __attribute__((aligned(16))) float As[2][kBK * LA];
    __shared__ __attribute__((aligned(16))) float Bs[2][kBK * LB];
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const int wm = wave / 2, wn = wave % 2;
    const int64_t m0 = (int64_t)bx * BM;
    const int n0 = by * BN;
    const int64_t k_lo = (int64_t)bz * op.k_chunk;
    const int64_t k_hi = (k_lo + op.k_chunk < op.K) ? (k_lo + op.k_chunk) : op.K;
    const bool a_kfast = (op.sak == 1), b_kfast = (op.sbk == 1);
    const bool a_vec = FAST || (op.vec_a && (m0 + BM <= op.M)), b_vec = FAST || (op.vec_b && (n0 + BN <= op.N));

    floatx16 acc[2][WN];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < WN; ++ni)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mi][ni][i] = 0.f;

    float ra[EA], rb[EB];
    // one operand tile [rows x kBK] -> registers.  vec: float4 along the contiguous dimension
    auto load_op = [&](const float *__restrict__ P, int64_t srow, int64_t sk, bool kfast, bool vec, int64_t row0,
                       int64_t nrows_total, int64_t kt, auto &r, auto rows_c, auto elems_c) {
        constexpr int ROWS = decltype(rows_c)::value, E = decltype(elems_c)::value;
        if (FAST || (vec && kt + kBK <= k_hi)) {
            if (kfast) {                                   // 4 lanes cover the 16 k of one row
                const float *src = P + (row0 + tid / 4) * srow + kt + (tid % 4) * 4;
#pragma unroll
                for (int q = 0; q < E / 4; ++q) {
                    const float4 v = *reinterpret_cast<const float4 *>(src + (int64_t)q * (kBlock / 4) * srow);
                    r[4 * q] = v.x; r[4 * q + 1] = v.y; r[4 * q + 2] = v.z; r[4 * q + 3] = v.w;
                }
            } else {                                       // ROWS/4 lanes cover one k
                const float *src = P + row0 + (tid % (ROWS / 4)) * 4 + (kt + tid / (ROWS / 4)) * sk;
#pragma unroll
                for (int q = 0; q < E / 4; ++q) {
                    const float4 v = *reinterpret_cast<const float4 *>(src + (int64_t)q * (kBlock / (ROWS / 4)) * sk);
                    r[4 * q] = v.x; r[4 * q + 1] = v.y; r[4 * q + 2] = v.z; r[4 * q + 3] = v.w;
                }
            }
        } else if constexpr (!FAST) {
#pragma unroll
            for (int q = 0; q < E; ++q) {
                const int e = tid + q * kBlock;
                const int kk = kfast ? (e % kBK) : (e / ROWS);
                const int rr = kfast ? (e / kBK) : (e % ROWS);
                const int64_t row = row0 + rr, k = kt + kk;
                r[q] = (row < nrows_total && k < k_hi) ? P[row * srow + k * sk] : 0.f;
            }
        }
    };
    auto store_op = [&](float *__restrict__ S, int ld, bool kfast, bool vec, bool full, auto &r, auto rows_c,
                        auto elems_c) {
        constexpr int ROWS = decltype(rows_c)::value, E = decltype(elems_c)::value;
        if (FAST || (vec && full)) {
            if (kfast) {
#pragma unroll
                for (int q = 0; q < E / 4; ++q) {
                    const int row = tid / 4 + q * (kBlock / 4), k = (tid % 4) * 4;
#pragma unroll
                    for (int t = 0; t < 4; ++t) S[(k + t) * ld + row] = r[4 * q + t];
                }
            } else {
#pragma unroll
                for (int q = 0; q < E / 4; ++q) {
                    const int row = (tid % (ROWS / 4)) * 4, k = tid / (ROWS / 4) + q * (kBlock / (ROWS / 4));
                    *reinterpret_cast<float4 *>(S + k * ld + row) = make_float4(r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]);
                }
            }
        } else if constexpr (!FAST) {
#pragma unroll
            for (int q = 0; q < E; ++q) {
                const int e = tid + q * kBlock;
                const int kk = kfast ? (e % kBK) : (e / ROWS);
                const int rr = kfast ? (e / kBK) : (e % ROWS);
                S[kk * ld + rr] = r[q];
            }
        }
    };
    using RA = std::integral_constant<int, BM>; using RB = std::integral_constant<int, BN>;
    using NA = std::integral_constant<int, EA>; using NB = std::integral_constant<int, EB>;

    if (k_lo < k_hi) {
        load_op(op.A, op.sam, op.sak, a_kfast, a_vec, m0, op.M, k_lo, ra, RA{}, NA{});
        load_op(op.B, op.sbn, op.sbk, b_kfast, b_vec, (int64_t)n0, (int64_t)op.N, k_lo, rb, RB{}, NB{});
        store_op(As[0], LA, a_kfast, a_vec, k_lo + kBK <= k_hi, ra, RA{}, NA{});
        store_op(Bs[0], LB, b_kfast, b_vec, k_lo + kBK <= k_hi, rb, RB{}, NB{});
        __syncthreads();
        int cur = 0;
        for (int64_t kt = k_lo; kt < k_hi; kt += kBK) {
            const bool more = kt + kBK < k_hi;
            if (more) {
                load_op(op.A, op.sam, op.sak, a_kfast, a_vec, m0, op.M, kt + kBK, ra, RA{}, NA{});
                load_op(op.B, op.sbn, op.sbk, b_kfast, b_vec, (int64_t)n0, (int64_t)op.N, kt + kBK, rb, RB{}, NB{});
            }
            const float *as = As[cur] + (lane / 32) * LA + wm * 64 + lane % 32;
            const float *bs = Bs[cur] + (lane / 32) * LB + wn * 32 * WN + lane % 32;
            float a[2][2], b[2][WN];          // fragments of k-step s live in slot s&1: the next step's LDS
#pragma unroll                                // reads are issued before this step's MFMAs
            for (int mi = 0; mi < 2; ++mi) a[0][mi] = as[mi * 32];
#pragma unroll
            for (int ni = 0; ni < WN; ++ni) b[0][ni] = bs[ni * 32];
#pragma unroll
            for (int ks = 0; ks < kBK / 2; ++ks) {
                const int c = ks & 1, nx = c ^ 1;
                if (ks + 1 < kBK / 2) {
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi) a[nx][mi] = as[(2 * ks + 2) * LA + mi * 32];
#pragma unroll
                    for (int ni = 0; ni < WN; ++ni) b[nx][ni] = bs[(2 * ks + 2) * LB + ni * 32];
                }
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < WN; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c][mi], b[c][ni], acc[mi][ni], 0, 0, 0);
            }
            if (more) {                                    // the other stage: nobody reads it now
                const bool full = kt + 2 * kBK <= k_hi;
                store_op(As[cur ^ 1], LA, a_kfast, a_vec, full, ra, RA{}, NA{});
                store_op(Bs[cur ^ 1], LB, b_kfast, b_vec, full, rb, RB{}, NB{});
            }
            __syncthreads();
            cur ^= 1;
        }
    }

    gemm_epilogue<WN, EPI, FAST, DROP>(op, acc, m0, n0, wm, wn, lane, bz);
}

template <int WN, int EPI, bool FAST, bool DROP>
__global__ __launch_bounds__(kBlock) void k_gemm(GemmOp op) {
    gemm_f32_tile<WN, EPI, FAST, DROP>(op, blockIdx.x, blockIdx.y, blockIdx.z);
}
// Two independent products in ONE launch (round 6): the user side's and the item side's table products of a NeuMF step are
// each ~100 workgroups of 16 dependent k steps - latency-bound, 29-34 us per launch whatever the loader.  Side by side
// (workgroups [0, ax) take `a`, the rest `b`; k slices beyond a product's own count leave at once) the pair costs what one did.
template <int WN, int EPI>
__global__ __launch_bounds__(kBlock) void k_gemm_pair(GemmOp a, GemmOp b, unsigned ax, unsigned az, unsigned bz_n) {
    if (blockIdx.x < ax) { if (blockIdx.z < az) gemm_f32_tile<WN, EPI, false, false>(a, blockIdx.x, blockIdx.y, blockIdx.z); }
    else if (blockIdx.z < bz_n) gemm_f32_tile<WN, EPI, false, false>(b, blockIdx.x - ax, blockIdx.y, blockIdx.z);
}

// ---------------------------------------------------------------------------------------------
// bf16-input variant (throughput mode; BASELINE configs[3] names it): operands stay fp32 in HBM, are
// rounded to bf16 (nearest-even) on their way into LDS and multiplied by v_mfma_f32_32x32x16_bf16
// (fp32 accumulate, 16x the fp32 MFMA rate).  LDS tiles are row-major with k contiguous - a lane's
// fragment is 8 consecutive k = one 16-byte read - at an 80-byte row pitch (odd multiple of 16 B:
// conflict free).  Interior, aligned tiles only (launch_gemm falls back to the fp32 kernel otherwise).
// ---------------------------------------------------------------------------------------------
constexpr int kBK16 = 32, kLdk16 = kBK16 + 8;


template <int WN, int EPI, bool DROP>
__global__ __launch_bounds__(kBlock) void k_gemm_bf16(GemmOp op) {
    constexpr int BM = kGemmBM, BN = 64 * WN;
    constexpr int QA = BM * kBK16 / kBlock / 4, QB = BN * kBK16 / kBlock / 4;      // float4 loads per thread per tile
    __shared__ __attribute__((aligned(16))) uint16_t As[2][BM * kLdk16];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[2][BN * kLdk16];
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const int wm = wave / 2, wn = wave % 2;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int64_t k_lo = (int64_t)blockIdx.z * op.k_chunk;
    const int64_t k_hi = (k_lo + op.k_chunk < op.K) ? (k_lo + op.k_chunk) : op.K;
    const bool a_kfast = (op.sak == 1), b_kfast = (op.sbk == 1);

    floatx16 acc[2][WN];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < WN; ++ni)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mi][ni][i] = 0.f;

    float ra[4 * QA], rb[4 * QB];
    // k-contiguous operand: float4 along k (8 lanes cover the 32 k of a row).  Operand contiguous along
    // its rows (the weight-gradient GEMM's two operands, W in the d-input GEMM): a thread takes ONE row
    // and 4*Q consecutive k with scalar loads - each wave instruction still reads 64 consecutive rows of
    // one k, 256 contiguous bytes - so that its bf16 pack is k-contiguous and lands in LDS as 16-byte
    // writes (a float4 along the rows would have to be scattered with 2-byte stores).
    auto load_op = [&](const float *__restrict__ P, int64_t srow, int64_t sk, bool kfast, int64_t row0, int64_t kt,
                       auto &r, auto rows_c, auto q_c) {
        constexpr int ROWS = decltype(rows_c)::value, Q = decltype(q_c)::value;
        if (kfast) {
            const float *src = P + (row0 + tid / 8) * srow + kt + (tid % 8) * 4;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const float4 v = *reinterpret_cast<const float4 *>(src + (int64_t)q * (kBlock / 8) * srow);
                r[4 * q] = v.x; r[4 * q + 1] = v.y; r[4 * q + 2] = v.z; r[4 * q + 3] = v.w;
            }
        } else {
            const float *src = P + row0 + (tid % ROWS) + (kt + (int64_t)(tid / ROWS) * (4 * Q)) * sk;
#pragma unroll
            for (int q = 0; q < 4 * Q; ++q) r[q] = src[(int64_t)q * sk];
        }
    };
    auto pack2 = [](float lo, float hi) { return bf16_pack2(lo, hi); };
    auto store_op = [&](uint16_t *__restrict__ S, bool kfast, auto &r, auto rows_c, auto q_c) {
        constexpr int ROWS = decltype(rows_c)::value, Q = decltype(q_c)::value;
        if (kfast) {
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int row = tid / 8 + q * (kBlock / 8), k = (tid % 8) * 4;
                *reinterpret_cast<uint2 *>(S + row * kLdk16 + k) =
                    make_uint2(pack2(r[4 * q], r[4 * q + 1]), pack2(r[4 * q + 2], r[4 * q + 3]));
            }
        } else {
            uint16_t *dst = S + (tid % ROWS) * kLdk16 + (tid / ROWS) * (4 * Q);
#pragma unroll
            for (int q = 0; q < Q / 2; ++q)
                *reinterpret_cast<uint4 *>(dst + 8 * q) =
                    make_uint4(pack2(r[8 * q], r[8 * q + 1]), pack2(r[8 * q + 2], r[8 * q + 3]),
                               pack2(r[8 * q + 4], r[8 * q + 5]), pack2(r[8 * q + 6], r[8 * q + 7]));
        }
    };
    using RA = std::integral_constant<int, BM>; using RB = std::integral_constant<int, BN>;
    using NA = std::integral_constant<int, QA>; using NB = std::integral_constant<int, QB>;

    if (k_lo < k_hi) {
        load_op(op.A, op.sam, op.sak, a_kfast, m0, k_lo, ra, RA{}, NA{});
        load_op(op.B, op.sbn, op.sbk, b_kfast, (int64_t)n0, k_lo, rb, RB{}, NB{});
        store_op(As[0], a_kfast, ra, RA{}, NA{});
        store_op(Bs[0], b_kfast, rb, RB{}, NB{});
        __syncthreads();
        int cur = 0;
        for (int64_t kt = k_lo; kt < k_hi; kt += kBK16) {
            const bool more = kt + kBK16 < k_hi;
            if (more) {
                load_op(op.A, op.sam, op.sak, a_kfast, m0, kt + kBK16, ra, RA{}, NA{});
                load_op(op.B, op.sbn, op.sbk, b_kfast, (int64_t)n0, kt + kBK16, rb, RB{}, NB{});
            }
            const uint16_t *as = As[cur] + (wm * 64 + lane % 32) * kLdk16 + (lane / 32) * 8;
            const uint16_t *bs = Bs[cur] + (wn * 32 * WN + lane % 32) * kLdk16 + (lane / 32) * 8;
#pragma unroll
            for (int ks = 0; ks < kBK16 / 16; ++ks) {
                bf16x8 a[2], b[WN];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
                    a[mi] = *reinterpret_cast<const bf16x8 *>(as + mi * 32 * kLdk16 + ks * 16);
#pragma unroll
                for (int ni = 0; ni < WN; ++ni)
                    b[ni] = *reinterpret_cast<const bf16x8 *>(bs + ni * 32 * kLdk16 + ks * 16);
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < WN; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
            }
            if (more) {
                store_op(As[cur ^ 1], a_kfast, ra, RA{}, NA{});
                store_op(Bs[cur ^ 1], b_kfast, rb, RB{}, NB{});
            }
            __syncthreads();
            cur ^= 1;
        }
    }
    gemm_epilogue<WN, EPI, true, DROP>(op, acc, m0, n0, wm, wn, lane, blockIdx.z);
}

// bf16-STORAGE variant (precision level 2): both operands are bf16 in HBM, so a tile row of 32 k is 64 bytes -
// 4 lanes x 16 bytes, copied to LDS as they are (no conversion, half the operand bytes of the fp32-storage
// kernels above, which is what bounded them).  Operands that are contiguous along their rows instead of k (the
// weight-gradient GEMM) keep that layout in LDS and are transposed by the fragment read (lds_frag_tr below).
// Epilogues: bias + ReLU (+dropout) or gate with bf16 output (round to nearest even), or fp32 atomics (split-K).

// Which tile a workgroup computes.  Workgroups go to the 8 XCDs round-robin by their linear id (observed, used for
// speed only), and each XCD has its own L2: tiles that read the same operand panel are given to workgroups that
// land on ONE XCD next to each other in time, so the panel comes from HBM once and from that L2 afterwards.
//   one k range (forward, input gradient): the column tiles of one 128-row panel of A share it;
//   split-K (weight gradient): all tiles of one k chunk share the chunk's two panels.
struct TileId { unsigned x, y, z; };
__device__ __forceinline__ TileId tile_of_block() {
    const unsigned gx = gridDim.x, gy = gridDim.y, gz = gridDim.z;
    TileId t{blockIdx.x, blockIdx.y, blockIdx.z};
    const unsigned lin = t.x + gx * (t.y + gy * t.z), xcd = lin % 8, slot = lin / 8;
    if (gz > 1) {
        if (gz % 8 == 0) {
            const unsigned per = gx * gy, r = slot % per;
            t.z = (slot / per) * 8 + xcd; t.x = r % gx; t.y = r / gx;
        }
    } else if (gx % 8 == 0) {
        t.y = slot % gy; t.x = (slot / gy) * 8 + xcd;
    }
    return t;
}

constexpr int kBKH = DAISY_BKH, kLdkH = kBKH;          // k depth of a tile (64: 587 vs 610 TFLOP/s on the forward shape, step equal -
                                                // 64 KB of LDS per workgroup halve the resident workgroups).  k-contiguous tiles
                                                // are unpadded (64-byte rows); the four 16-byte chunks of row r sit at
                                                // position chunk ^ ((r / 4) % 4): the fragment reads (ds_read_b128: 16 rows
                                                // per LDS cycle) and the tile writes (two rows per 8-lane group) are then
                                                // both conflict-free; the first version's 80-byte pitch left 31 % of the LDS
                                                // cycles in bank conflicts (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE)
// (32-deep tiles: 4 chunks per 64-byte row, chunk ^ ((r / 4) % 4); 64-deep: 8 chunks per 128-byte row, chunk ^ ((r / 2) % 8))
__device__ __forceinline__ int swz_of_row(int row) { return kBKH == 32 ? ((row >> 2) & 3) : ((row >> 1) & 7); }
__device__ __forceinline__ int swz_chunk(int row, int chunk) { return chunk ^ swz_of_row(row); }
// An operand that is contiguous along its ROWS instead of k (both operands of the weight-gradient GEMM: dZ^T and
// X^T with k = the batch row) is copied to LDS as it lies in memory - [k][row] tiles, 16-byte loads along the rows -
// and the MFMA fragment (8 consecutive k of one row per lane) comes out of gfx950's transposing LDS read:
// ds_read_b64_tr_b16 hands lane i of a 16-lane group column i of the [4 k][16 rows] block whose 16 four-element
// pieces the lanes address (measured: result[i][j] = piece[4j + i/4][i%4]), two of them per fragment.  The first
// version read such operands with 2-byte global loads and packed them in registers: 265 TFLOP/s on the weight
// gradients against 430-600 on the k-contiguous GEMMs.  Pitch rows + 32 halfwords: the 8 k rows one instruction
// touches fall on 4 distinct 16-bank offsets, twice - the two LDS cycles its 512 bytes need anyway.
constexpr int kPadT = 32;

template <int WN, int EPI, bool DROP, bool AK, bool BK>      // AK / BK: operand A / B is contiguous along k (else along its rows)
__global__ __launch_bounds__(kBlock) void k_gemm_h(GemmOp op) {
    constexpr int BM = kGemmBM, BN = 64 * WN;
    constexpr int LPT = kBKH / 8;                               // k-contiguous: lanes per tile row (16 bytes each)
    constexpr int RPP = kBlock / LPT;                           //               tile rows per pass of the workgroup
    constexpr int PTA = BM + kPadT, PTB = BN + kPadT;           // row-contiguous: halfwords per k row of the LDS tile
    constexpr int kTileA = AK ? BM * kLdkH : kBKH * PTA, kTileB = BK ? BN * kLdkH : kBKH * PTB;
    // one LDS block: two stages of the A and B tiles; the output tile of the bf16 epilogues reuses it afterwards
    constexpr int kStage = 2 * (kTileA + kTileB), kOut = BM * (BN + 8);
    __shared__ __attribute__((aligned(16))) uint16_t smem[kStage > kOut ? kStage : kOut];
    uint16_t *const As0 = smem, *const Bs0 = smem + 2 * kTileA;
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const int wm = wave / 2, wn = wave % 2;
    const TileId tile = tile_of_block();
    const int64_t m0 = (int64_t)tile.x * BM;
    const int n0 = tile.y * BN;
    const int64_t k_lo = (int64_t)tile.z * op.k_chunk;
    const int64_t k_hi = (k_lo + op.k_chunk < op.K) ? (k_lo + op.k_chunk) : op.K;

    floatx16 acc[2][WN];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < WN; ++ni)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mi][ni][i] = 0.f;

    // registers of one tile: 16 bytes per load in both layouts (BM*32*2 / 256 threads = 2 loads for 128 rows)
    // (clang's own vector type: arrays of HIP's uint4 class are not split into registers and went through scratch)
    constexpr int NQ = BM * kBKH / 8 / kBlock;
    u32x4 ra[NQ], rb[NQ];
    auto load_op = [&](const uint16_t *__restrict__ P, int64_t srow, int64_t sk, auto kfast_c, int64_t row0, int64_t kt,
                       auto &r, auto rows_c) {
        constexpr int ROWS = decltype(rows_c)::value;
        if constexpr (decltype(kfast_c)::value) {
            const uint16_t *src = P + (row0 + tid / LPT) * srow + kt + (tid % LPT) * 8;
#pragma unroll
            for (int q = 0; q < ROWS / RPP; ++q) r[q] = *reinterpret_cast<const u32x4 *>(src + (int64_t)q * RPP * srow);
        } else {
            constexpr int VPR = ROWS / 8, KPP = kBlock / VPR;      // 16-byte vectors per k row; k rows per pass
            const uint16_t *src = P + row0 + (tid % VPR) * 8 + (kt + tid / VPR) * sk;
#pragma unroll
            for (int q = 0; q < kBKH / KPP; ++q) r[q] = *reinterpret_cast<const u32x4 *>(src + (int64_t)q * KPP * sk);
        }
    };
    auto store_op = [&](uint16_t *__restrict__ S, auto kfast_c, const auto &r, auto rows_c) {
        constexpr int ROWS = decltype(rows_c)::value;
        if constexpr (decltype(kfast_c)::value) {
#pragma unroll
            for (int q = 0; q < ROWS / RPP; ++q) {
                const int row = tid / LPT + q * RPP;
                *reinterpret_cast<u32x4 *>(S + row * kLdkH + swz_chunk(row, tid % LPT) * 8) = r[q];
            }
        } else {
            constexpr int VPR = ROWS / 8, KPP = kBlock / VPR, PT = ROWS + kPadT;
#pragma unroll
            for (int q = 0; q < kBKH / KPP; ++q)
                *reinterpret_cast<u32x4 *>(S + (tid / VPR + q * KPP) * PT + (tid % VPR) * 8) = r[q];
        }
    };
    using RA = std::integral_constant<int, BM>; using RB = std::integral_constant<int, BN>;
    using KA = std::integral_constant<bool, AK>; using KB = std::integral_constant<bool, BK>;
    static_assert(BN <= BM, "tile registers are sized by the A tile");

    if (k_lo < k_hi) {
        load_op(op.A16, op.sam, op.sak, KA{}, m0, k_lo, ra, RA{});
        load_op(op.B16, op.sbn, op.sbk, KB{}, (int64_t)n0, k_lo, rb, RB{});
        store_op(As0, KA{}, ra, RA{});
        store_op(Bs0, KB{}, rb, RB{});
        __syncthreads();
        int cur = 0;
        for (int64_t kt = k_lo; kt < k_hi; kt += kBKH) {
            const bool more = kt + kBKH < k_hi;
            if (more) {
                load_op(op.A16, op.sam, op.sak, KA{}, m0, kt + kBKH, ra, RA{});
                load_op(op.B16, op.sbn, op.sbk, KB{}, (int64_t)n0, kt + kBKH, rb, RB{});
            }
            const uint16_t *At = As0 + cur * kTileA, *Bt = Bs0 + cur * kTileB;
            // k-contiguous tile: lane -> row lane%32, k half lane/32.  [k][row] tile: the address of this lane's piece
            // of the transposing read (k row 8*(lane/32) + (lane%16)/4, rows 16*((lane%32)/16) + 4*(lane%4) ...)
            // (the row offsets wm*64 + mi*32 and wn*32*WN + ni*32 are multiples of 32: the swizzle of a lane's row
            // depends on lane % 32 only)
            const int sw = swz_of_row(lane % 32), half = lane / 32;
            const uint16_t *as = AK ? At + (wm * 64 + lane % 32) * kLdkH
                                    : At + (8 * (lane / 32) + (lane % 16) / 4) * PTA + wm * 64 + 16 * ((lane % 32) / 16) + 4 * (lane % 4);
            const uint16_t *bs = BK ? Bt + (wn * 32 * WN + lane % 32) * kLdkH
                                    : Bt + (8 * (lane / 32) + (lane % 16) / 4) * PTB + wn * 32 * WN + 16 * ((lane % 32) / 16) + 4 * (lane % 4);
#pragma unroll
            for (int ks = 0; ks < kBKH / 16; ++ks) {
                bf16x8 a[2], b[WN];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) {
                    if constexpr (AK) a[mi] = *reinterpret_cast<const bf16x8 *>(as + mi * 32 * kLdkH + ((2 * ks + half) ^ sw) * 8);
                    else a[mi] = lds_frag_tr(as + ks * 16 * PTA + mi * 32, PTA);
                }
#pragma unroll
                for (int ni = 0; ni < WN; ++ni) {
                    if constexpr (BK) b[ni] = *reinterpret_cast<const bf16x8 *>(bs + ni * 32 * kLdkH + ((2 * ks + half) ^ sw) * 8);
                    else b[ni] = lds_frag_tr(bs + ks * 16 * PTB + ni * 32, PTB);
                }
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < WN; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
            }
            if (more) {
                store_op(As0 + (cur ^ 1) * kTileA, KA{}, ra, RA{});
                store_op(Bs0 + (cur ^ 1) * kTileB, KB{}, rb, RB{});
            }
            __syncthreads();
            cur ^= 1;
        }
    }
    if (EPI == EPI_ATOMIC || op.C16 == nullptr) {      // fp32 result: split-K atomics, or the tower's input gradient
        gemm_epilogue<WN, EPI, true, DROP>(op, acc, m0, n0, wm, wn, lane, tile.z);
    } else {        // bf16 output (interior tiles only: launch_gemm_h checks)
        // The MFMA result layout gives a lane ONE column and 32 scattered rows: written directly that is 64 two-byte
        // stores per lane.  So the tile takes a detour through LDS (the operand stages are dead by now) and
        // leaves as 16-byte stores along its rows.
        constexpr int LDT = BN + 8;                                       // halfwords per staged row (16-byte multiple)
        uint16_t *Ts = smem;              // (the last k iteration ended with a barrier: every fragment read is done)
        const uint16_t *__restrict__ Gt = (EPI == EPI_GATE && op.G16) ? op.G16 + m0 * op.ldg + n0 : nullptr;
        const int ldg = (int)op.ldg;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < WN; ++ni) {
                const int nl = wn * 32 * WN + ni * 32 + lane % 32;
                float bias = 0.f;
                if constexpr (EPI == EPI_BIAS_RELU) bias = op.bias[n0 + nl];
#pragma unroll
                for (int i = 0; i < 16; i += 2) {                       // rows ml, ml + 1 of column nl: one packed conversion
                    const int ml = wm * 64 + mi * 32 + (i / 4) * 8 + (lane / 32) * 4 + (i % 4);
                    float v[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        v[h] = acc[mi][ni][i + h];
                        if constexpr (EPI == EPI_BIAS_RELU) v[h] = fmaxf(v[h] + bias, 0.f);
                        if constexpr (DROP)
                            if (op.drop_thresh)
                                v[h] = drop_keep(op.drop_seed, op.drop_stream,
                                                 (uint64_t)(m0 + ml + h) * (uint64_t)op.N + (uint64_t)(n0 + nl), op.drop_thresh)
                                           ? v[h] * op.drop_scale : 0.f;
                    }
                    const uint32_t pk = bf16_pack2(v[0], v[1]);
                    Ts[ml * LDT + nl] = (uint16_t)pk;
                    Ts[(ml + 1) * LDT + nl] = (uint16_t)(pk >> 16);
                }
            }
        __syncthreads();
        constexpr int VPR = BN / 8;                                       // 16-byte vectors per tile row
        uint16_t *__restrict__ Ct = op.C16 + m0 * op.ldc + n0;
        for (int e = tid; e < BM * VPR; e += kBlock) {
            const int row = e / VPR, c8 = (e % VPR) * 8;
            uint4 v = *reinterpret_cast<const uint4 *>(Ts + row * LDT + c8);
            if constexpr (EPI == EPI_GATE) {
                if (Gt) {                                                 // gate: x > 0 of the layer input, 8 columns at a time
                    const uint4 gq = *reinterpret_cast<const uint4 *>(Gt + (int64_t)row * ldg + c8);
                    const uint32_t gw[4] = {gq.x, gq.y, gq.z, gq.w};
                    uint32_t vw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const uint16_t g0 = (uint16_t)gw[q], g1 = (uint16_t)(gw[q] >> 16);
                        float lo = bf16_positive(g0) ? bf16_to_f32((uint16_t)vw[q]) * op.gate_scale : 0.f;
                        float hi = bf16_positive(g1) ? bf16_to_f32((uint16_t)(vw[q] >> 16)) * op.gate_scale : 0.f;
                        vw[q] = bf16_pack2(lo, hi);
                    }
                    v = make_uint4(vw[0], vw[1], vw[2], vw[3]);
                }
            }
            *reinterpret_cast<uint4 *>(Ct + (int64_t)row * op.ldc + c8) = v;
        }
    }
}

// shapes the bf16-storage kernel takes: whole tiles, k ranges in multiples of 32, 16-byte aligned rows
bool gemm_h_ok(const GemmOp &op) {
    const int bn = (op.N > 64) ? 128 : 64;
    const int64_t splits = (op.k_chunk < op.K) ? (op.K + op.k_chunk - 1) / op.k_chunk : 1;
    auto al = [](const uint16_t *p, int64_t srow, int64_t sk) {
        if (((uintptr_t)p & 15) != 0) return false;
        return sk == 1 ? (srow % 8 == 0) : (srow == 1 && sk % 8 == 0);     // 16-byte loads along k / along the rows
    };
    if (op.sak != 1 && op.sbk == 1) return false;          // (A along rows, B along k) is not a layout of the tower
    return op.M % kGemmBM == 0 && op.N % bn == 0 && op.K % kBKH == 0 && (splits == 1 || op.k_chunk % kBKH == 0) &&
           al(op.A16, op.sam, op.sak) && al(op.B16, op.sbn, op.sbk);
}

// k slices of an op, and its k_chunk clamped to K (the first thing every resolve step does)
static unsigned take_splits(GemmOp &op) {
    const int64_t splits = (op.k_chunk < op.K) ? (op.K + op.k_chunk - 1) / op.k_chunk : 1;
    if (op.k_chunk >= op.K) op.k_chunk = op.K;
    return (unsigned)splits;
}
static bool epi_can_drop(int epi) { return epi == EPI_BIAS_RELU || epi == EPI_GATE; }

GemmPath resolve_gemm_h(GemmOp &op, int epi) {
    GemmPath p{};
    p.family = GEMM_H;
    p.splits = take_splits(op);
    p.wn = (op.N > 64) ? 2 : 1;
    p.gx = (unsigned)(op.M / kGemmBM); p.gy = (unsigned)(op.N / (64 * p.wn));
    p.drop = epi_can_drop(epi) && op.drop_thresh != 0;
    // the three operand layouts the tower uses: forward X (k) x W (k), input gradient dZ (k) x W^T (rows), weight
    // gradient dZ^T (rows) x X^T (rows); (rows, k) is refused by gemm_h_ok
    p.ak = op.sak == 1;
    p.bk = p.ak && op.sbk == 1;
    return p;
}

template <int EPI>
static void run_gemm_h(const GemmOp &op, const GemmPath &p, hipStream_t s) {
    const dim3 grid(p.gx, p.gy, p.splits);
    constexpr bool can_drop = (EPI == EPI_BIAS_RELU || EPI == EPI_GATE);
    auto go = [&](auto wn_c, auto drop_c, auto ak_c, auto bk_c) {
        hipLaunchKernelGGL((k_gemm_h<decltype(wn_c)::value, EPI, decltype(drop_c)::value, decltype(ak_c)::value,
                                     decltype(bk_c)::value>), grid, dim3(kBlock), 0, s, op);
    };
    using T = std::true_type; using F = std::false_type;
    using W1 = std::integral_constant<int, 1>; using W2 = std::integral_constant<int, 2>;
    auto go2 = [&](auto wn_c, auto drop_c) {
        if (p.ak && p.bk) go(wn_c, drop_c, T{}, T{});
        else if (p.ak) go(wn_c, drop_c, T{}, F{});
        else go(wn_c, drop_c, F{}, F{});
    };
    if (p.wn == 2) {
        if constexpr (can_drop) { if (p.drop) go2(W2{}, T{}); else go2(W2{}, F{}); } else go2(W2{}, F{});
    } else {
        if constexpr (can_drop) { if (p.drop) go2(W1{}, T{}); else go2(W1{}, F{}); } else go2(W1{}, F{});
    }
}

template <int EPI>
void launch_gemm_h(GemmOp op, hipStream_t s) {
    const GemmPath p = resolve_gemm_h(op, EPI);
    run_gemm_h<EPI>(op, p, s);
}

// fp32 -> bf16 (round to nearest even): the per-step copy of the MLP weights, [rows][cols] as stored and (yt)
// transposed, so that the forward GEMM and the input-gradient GEMM both read W along their k
__global__ void k_to_bf16(const float *__restrict__ x, int64_t n, int cols, uint16_t *__restrict__ y,
                          uint16_t *__restrict__ yt) {
    const int64_t rows = n / cols;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const uint16_t h = (uint16_t)bf16_rne(x[e]);
        y[e] = h;
        yt[(e % cols) * rows + e / cols] = h;
    }
}
void to_bf16_and_transpose(const float *x, int64_t n, int cols, uint16_t *y, uint16_t *yt, hipStream_t s) {
    hipLaunchKernelGGL(k_to_bf16, dim3(grid_for(n, kBlock * 4)), dim3(kBlock), 0, s, x, n, cols, y, yt);
}

// float4 path preconditions: unit stride along one dimension, the other stride and the base 16-byte aligned
static bool vec_ok(const float *p, int64_t s_row, int64_t s_k, int64_t k_chunk) {
    if (((uintptr_t)p & 15) != 0) return false;
    if (s_k == 1) return s_row % 4 == 0 && k_chunk % 4 == 0;
    if (s_row == 1) return s_k % 4 == 0;
    return false;
}

// the part of the decision k_gemm and k_gemm_pair share: slices, float4 eligibility, tile width, row and column tiles
static GemmPath resolve_f32_tiles(GemmOp &op) {
    GemmPath p{};
    p.splits = take_splits(op);
    op.vec_a = vec_ok(op.A, op.sam, op.sak, p.splits > 1 ? op.k_chunk : 4);
    op.vec_b = vec_ok(op.B, op.sbn, op.sbk, p.splits > 1 ? op.k_chunk : 4);
    p.wn = (op.N > 64) ? 2 : 1;
    const int bn = 64 * p.wn;
    p.gx = (unsigned)((op.M + kGemmBM - 1) / kGemmBM); p.gy = (unsigned)((op.N + bn - 1) / bn);
    return p;
}

GemmPath resolve_gemm(GemmOp &op, int epi) {
    GemmPath p = resolve_f32_tiles(op);
    p.fast = op.vec_a && op.vec_b && op.M % kGemmBM == 0 && op.N % (64 * p.wn) == 0 && op.K % kBK == 0 &&
             (p.splits == 1 || op.k_chunk % kBK == 0);
    const bool bf16 = op.bf16 && p.fast && op.K % kBK16 == 0 && (p.splits == 1 || op.k_chunk % kBK16 == 0);
    p.family = bf16 ? GEMM_BF16IN : GEMM_F32;
    p.drop = epi_can_drop(epi) && op.drop_thresh != 0;
    return p;
}

template <int EPI>
static void run_gemm(const GemmOp &op, const GemmPath &p, hipStream_t s) {
    const dim3 grid(p.gx, p.gy, p.splits);
    auto go = [&](auto wn_c, auto fast_c, auto drop_c) {
        if (p.family == GEMM_BF16IN)
            hipLaunchKernelGGL((k_gemm_bf16<decltype(wn_c)::value, EPI, decltype(drop_c)::value>), grid, dim3(kBlock), 0,
                               s, op);
        else
            hipLaunchKernelGGL((k_gemm<decltype(wn_c)::value, EPI, decltype(fast_c)::value, decltype(drop_c)::value>),
                               grid, dim3(kBlock), 0, s, op);
    };
    using T = std::true_type; using F = std::false_type;
    using W1 = std::integral_constant<int, 1>; using W2 = std::integral_constant<int, 2>;
    constexpr bool can_drop = (EPI == EPI_BIAS_RELU || EPI == EPI_GATE);
    if (p.wn == 2) {
        if (p.fast) { if constexpr (can_drop) { if (p.drop) go(W2{}, T{}, T{}); else go(W2{}, T{}, F{}); } else go(W2{}, T{}, F{}); }
        else        { if constexpr (can_drop) { if (p.drop) go(W2{}, F{}, T{}); else go(W2{}, F{}, F{}); } else go(W2{}, F{}, F{}); }
    } else {
        if (p.fast) { if constexpr (can_drop) { if (p.drop) go(W1{}, T{}, T{}); else go(W1{}, T{}, F{}); } else go(W1{}, T{}, F{}); }
        else        { if constexpr (can_drop) { if (p.drop) go(W1{}, F{}, T{}); else go(W1{}, F{}, F{}); } else go(W1{}, F{}, F{}); }
    }
}

template <int EPI>
void launch_gemm(GemmOp op, hipStream_t s) {
    const GemmPath p = resolve_gemm(op, EPI);
    run_gemm<EPI>(op, p, s);
}

// the fp32 product of gemm.h (csrc/vae.hip's layers): k_gemm with plain stores, or its split-k slices stored apart
void gemm_f32(const float *A, int64_t sam, int64_t sak, const float *B, int64_t sbn, int64_t sbk, float *C, int64_t ldc,
              int64_t M, int N, int64_t K, int64_t k_chunk, int64_t slice_stride, hipStream_t s) {
    GemmOp op{};
    op.A = A; op.sam = sam; op.sak = sak;
    op.B = B; op.sbn = sbn; op.sbk = sbk;
    op.C = C; op.ldc = ldc; op.M = M; op.N = N; op.K = K; op.k_chunk = k_chunk;
    if (k_chunk < K) {
        op.slice_stride = slice_stride;
        launch_gemm<EPI_ATOMIC>(op, s);
    } else {
        launch_gemm<EPI_STORE>(op, s);
    }
}


// two products of the same (N, tile width) in one launch (k_gemm_pair): guarded-loader kernels, fp32
GemmPath resolve_gemm_pair(GemmOp &a, GemmOp &b) {
    GemmPath p = resolve_f32_tiles(a);            // (tile width and column tiles from a: the two share N)
    const GemmPath pb = resolve_f32_tiles(b);
    p.family = GEMM_PAIR;
    p.ax = p.gx;
    p.gx += pb.gx;
    p.splits_b = pb.splits;
    return p;
}

template <int EPI>
static void run_gemm_pair(const GemmOp &a, const GemmOp &b, const GemmPath &p, hipStream_t s) {
    const dim3 grid(p.gx, p.gy, p.splits > p.splits_b ? p.splits : p.splits_b);
    if (p.wn == 2) hipLaunchKernelGGL((k_gemm_pair<2, EPI>), grid, dim3(kBlock), 0, s, a, b, p.ax, p.splits, p.splits_b);
    else hipLaunchKernelGGL((k_gemm_pair<1, EPI>), grid, dim3(kBlock), 0, s, a, b, p.ax, p.splits, p.splits_b);
}

template <int EPI>
void launch_gemm_pair(GemmOp a, GemmOp b, hipStream_t s) {
    const GemmPath p = resolve_gemm_pair(a, b);
    run_gemm_pair<EPI>(a, b, p, s);
}

// daisy_gemm_case: one descriptor -> a GemmOp.  Everything a kernel would index is checked against the element counts
// the caller gave, and the shape against what the launcher takes, so that a wrong descriptor is an error return.
static int gemm_case_op(const daisy_gemm_desc &d, const char *w, GemmOp &op) {
    constexpr int64_t kMaxDim = (int64_t)1 << 24, kMaxStride = (int64_t)1 << 22;   // (products stay far inside int64; a
                                                                                    // tile's 32-bit offsets 127*ldc + 127*scn too)
    const int epi = d.epilogue;
    const bool h = d.launcher == DAISY_GEMM_LAUNCH_H, pair = d.launcher == DAISY_GEMM_LAUNCH_PAIR;
    DAISY_CHECK_ARG(d.launcher == DAISY_GEMM_LAUNCH || h || pair, "gemm_case: %s.launcher=%d", w, d.launcher);
    const bool inst = h ? (epi == EPI_BIAS_RELU || epi == EPI_GATE || epi == EPI_ATOMIC)
                        : pair ? (epi == EPI_STORE || epi == EPI_ATOMIC) : (epi >= EPI_STORE && epi <= EPI_ATOMIC);
    DAISY_CHECK_ARG(inst, "gemm_case: %s: launcher %d is not instantiated for epilogue %d", w, d.launcher, epi);
    DAISY_CHECK_ARG(d.M > 0 && d.M <= kMaxDim && d.N > 0 && d.N <= ((int64_t)1 << 20) && d.K > 0 && d.K <= kMaxDim,
                    "gemm_case: %s: M, N, K must be positive (and at most 2^24, 2^20, 2^24)", w);
    DAISY_CHECK_ARG(d.k_chunk > 0, "gemm_case: %s.k_chunk must be positive", w);
    DAISY_CHECK_ARG(d.A && d.B && d.C, "gemm_case: %s: A, B or C is NULL", w);
    auto stride_ok = [&](int64_t v) { return v > 0 && v <= kMaxStride; };
    DAISY_CHECK_ARG(stride_ok(d.sam) && stride_ok(d.sak), "gemm_case: %s.sam / sak out of range", w);
    DAISY_CHECK_ARG(stride_ok(d.sbn) && stride_ok(d.sbk), "gemm_case: %s.sbn / sbk out of range", w);
    DAISY_CHECK_ARG(stride_ok(d.ldc) && d.scn >= 0 && d.scn <= kMaxStride, "gemm_case: %s.ldc / scn out of range", w);
    const int64_t splits = (d.k_chunk < d.K) ? (d.K + d.k_chunk - 1) / d.k_chunk : 1;
    DAISY_CHECK_ARG(splits <= 0xFFF, "gemm_case: %s.k_chunk gives %lld slices (at most 4095)", w, (long long)splits);
    DAISY_CHECK_ARG(splits == 1 || epi == EPI_ATOMIC, "gemm_case: %s.k_chunk < K needs the ATOMIC epilogue", w);
    DAISY_CHECK_ARG(d.slice_stride >= 0 && d.slice_stride <= ((int64_t)1 << 40) && (d.slice_stride == 0 || epi == EPI_ATOMIC),
                    "gemm_case: %s.slice_stride is for the ATOMIC epilogue (and not negative)", w);
    DAISY_CHECK_ARG(d.drop_p >= 0.f && d.drop_p < 1.f && (d.drop_p == 0.f || epi_can_drop(epi)),
                    "gemm_case: %s.drop_p must be in [0, 1) and 0 unless the epilogue is BIAS_RELU or GATE", w);
    DAISY_CHECK_ARG(!d.bf16 || d.launcher == DAISY_GEMM_LAUNCH, "gemm_case: %s.bf16 is a flag of launch_gemm", w);
    const bool c16 = d.c_bf16 != 0;
    DAISY_CHECK_ARG(!c16 || (h && epi != EPI_ATOMIC), "gemm_case: %s.c_bf16 needs launch_gemm_h with BIAS_RELU or GATE", w);
    DAISY_CHECK_ARG(!c16 || d.scn <= 1, "gemm_case: %s.scn: the bf16 output has no transposed store", w);
    const int64_t scn = d.scn ? d.scn : 1;
    DAISY_CHECK_ARG((d.M - 1) * d.sam + (d.K - 1) * d.sak < d.n_A, "gemm_case: %s.n_A=%lld is short of the operand", w, (long long)d.n_A);
    DAISY_CHECK_ARG((d.N - 1) * d.sbn + (d.K - 1) * d.sbk < d.n_B, "gemm_case: %s.n_B=%lld is short of the operand", w, (long long)d.n_B);
    DAISY_CHECK_ARG((d.M - 1) * d.ldc + (d.N - 1) * scn + (splits - 1) * d.slice_stride < d.n_C,
                    "gemm_case: %s.n_C=%lld is short of the output (%lld slices)", w, (long long)d.n_C, (long long)splits);
    if (epi == EPI_BIAS_RELU) {
        DAISY_CHECK_ARG(d.bias, "gemm_case: %s.bias is NULL", w);
        DAISY_CHECK_ARG(d.N - 1 < d.n_bias, "gemm_case: %s.n_bias=%lld is short of N", w, (long long)d.n_bias);
    }
    const bool gated = epi == EPI_GATE && d.gate;
    if (gated) {
        DAISY_CHECK_ARG(stride_ok(d.ldg), "gemm_case: %s.ldg out of range", w);
        DAISY_CHECK_ARG((d.M - 1) * d.ldg + d.N - 1 < d.n_gate, "gemm_case: %s.n_gate=%lld is short of the gate", w, (long long)d.n_gate);
    }
    op = GemmOp{};
    op.sam = d.sam; op.sak = d.sak; op.sbn = d.sbn; op.sbk = d.sbk;
    op.ldc = d.ldc; op.scn = d.scn; op.ldg = d.ldg;
    op.M = d.M; op.N = (int)d.N; op.K = d.K; op.k_chunk = d.k_chunk; op.slice_stride = d.slice_stride;
    op.bias = d.bias; op.gate_scale = d.gate_scale; op.bf16 = d.bf16 ? 1 : 0;
    op.drop_thresh = keep_threshold(d.drop_p);
    op.drop_scale = op.drop_thresh ? 1.f / (1.f - d.drop_p) : 1.f;
    op.drop_seed = d.drop_seed; op.drop_stream = d.drop_stream;
    if (h) {
        op.A16 = static_cast<const uint16_t *>(d.A); op.B16 = static_cast<const uint16_t *>(d.B);
        if (c16) { op.C16 = static_cast<uint16_t *>(d.C); op.G16 = gated ? static_cast<const uint16_t *>(d.gate) : nullptr; }
        else { op.C = static_cast<float *>(d.C); op.gate = gated ? static_cast<const float *>(d.gate) : nullptr; }
        DAISY_CHECK_ARG(gemm_h_ok(op), "gemm_case: %s: launch_gemm_h needs M %% 128 == 0, N %% 64 == 0 (128 when N > 64), K and k_chunk "
                        "%% %d == 0, 16-byte aligned operands along k or along their rows, and not (A rows, B k)", w, kBKH);
        // (the bf16 epilogue leaves and reads its gate in 16-byte pieces along the rows)
        DAISY_CHECK_ARG(!c16 || (((uintptr_t)d.C & 15) == 0 && d.ldc % 8 == 0), "gemm_case: %s.C / ldc: the bf16 output needs 16-byte aligned rows", w);
        DAISY_CHECK_ARG(!(c16 && gated) || (((uintptr_t)d.gate & 15) == 0 && d.ldg % 8 == 0),
                        "gemm_case: %s.gate / ldg: the bf16 gate needs 16-byte aligned rows", w);
    } else {
        op.A = static_cast<const float *>(d.A); op.B = static_cast<const float *>(d.B);
        op.C = static_cast<float *>(d.C); op.gate = gated ? static_cast<const float *>(d.gate) : nullptr;
    }
    return DAISY_OK;
}

template void launch_gemm<EPI_STORE>(GemmOp, hipStream_t);
template void launch_gemm<EPI_BIAS_RELU>(GemmOp, hipStream_t);
template void launch_gemm<EPI_GATE>(GemmOp, hipStream_t);
template void launch_gemm<EPI_ATOMIC>(GemmOp, hipStream_t);
template void launch_gemm_h<EPI_BIAS_RELU>(GemmOp, hipStream_t);
template void launch_gemm_h<EPI_GATE>(GemmOp, hipStream_t);
template void launch_gemm_h<EPI_ATOMIC>(GemmOp, hipStream_t);
template void launch_gemm_pair<EPI_STORE>(GemmOp, GemmOp, hipStream_t);
template void launch_gemm_pair<EPI_ATOMIC>(GemmOp, GemmOp, hipStream_t);

}  // namespace daisy

using namespace daisy;

extern "C" {

int daisy_gemm_nt_bf16(const uint16_t *A, const uint16_t *B, uint16_t *C, int64_t M, int32_t N, int32_t K,
                       daisy_stream_t stream) {
    DAISY_CHECK_ARG(A && B && C && M > 0 && N > 0 && K > 0, "gemm_nt_bf16: bad argument");
    GemmOp op{};
    op.A16 = A; op.sam = K; op.sak = 1;
    op.B16 = B; op.sbn = K; op.sbk = 1;
    op.C16 = C; op.ldc = N;
    op.M = M; op.N = N; op.K = K; op.k_chunk = K;
    DAISY_CHECK_ARG(gemm_h_ok(op), "gemm_nt_bf16: needs M %% 128 == 0, N %% 64 == 0 (128 when N > 64), K %% 32 == 0, 16-byte aligned rows");
    launch_gemm_h<EPI_GATE>(op, as_stream(stream));          // no gate tensor: a plain bf16 store
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_gemm_tn_bf16(const uint16_t *At, const uint16_t *Bt, float *C, int64_t M, int32_t N, int64_t K,
                       int64_t k_chunk, daisy_stream_t stream) {
    DAISY_CHECK_ARG(At && Bt && C && M > 0 && N > 0 && K > 0 && k_chunk > 0, "gemm_tn_bf16: bad argument");
    GemmOp op{};                         // the weight-gradient layout: both operands [K][rows], rows contiguous
    op.A16 = At; op.sam = 1; op.sak = M;
    op.B16 = Bt; op.sbn = 1; op.sbk = N;
    op.C = C; op.ldc = N;
    op.M = M; op.N = N; op.K = K; op.k_chunk = k_chunk;
    DAISY_CHECK_ARG(gemm_h_ok(op), "gemm_tn_bf16: needs M %% 128 == 0, N %% 64 == 0 (128 when N > 64), K and k_chunk %% 32 == 0, "
                                   "M and N %% 8 == 0, 16-byte aligned operands");
    launch_gemm_h<EPI_ATOMIC>(op, as_stream(stream));
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}
int daisy_gemm_nt_f32(const float *A, const float *B, float *C, int64_t M, int32_t N, int32_t K,
                      daisy_stream_t stream) {
    return daisy_gemm_nt(A, B, C, M, N, K, 0, stream);
}

int daisy_gemm_nt(const float *A, const float *B, float *C, int64_t M, int32_t N, int32_t K, int32_t bf16,
                  daisy_stream_t stream) {
    DAISY_CHECK_ARG(A && B && C && M > 0 && N > 0 && K > 0, "gemm_nt: bad argument");
    GemmOp op{};
    op.bf16 = bf16 ? 1 : 0;
    op.A = A; op.sam = K; op.sak = 1;
    op.B = B; op.sbn = K; op.sbk = 1;
    op.C = C; op.ldc = N; op.M = M; op.N = N; op.K = K; op.k_chunk = K;
    launch_gemm<EPI_STORE>(op, as_stream(stream));
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_gemm_case(daisy_gemm_desc *a, daisy_gemm_desc *b, daisy_stream_t stream) {
    DAISY_CHECK_ARG(a, "gemm_case: NULL descriptor");
    DAISY_CHECK_ARG((a->launcher == DAISY_GEMM_LAUNCH_PAIR) == (b != nullptr), "gemm_case: launch_gemm_pair takes two descriptors, the others one");
    GemmOp oa, ob;
    int rc = gemm_case_op(*a, "a", oa);
    if (rc) return rc;
    hipStream_t s = as_stream(stream);
    const int epi = a->epilogue;
    if (b) {
        rc = gemm_case_op(*b, "b", ob);
        if (rc) return rc;
        DAISY_CHECK_ARG(b->launcher == DAISY_GEMM_LAUNCH_PAIR && b->epilogue == epi, "gemm_case: b.launcher / b.epilogue differ from a's");
        DAISY_CHECK_ARG(a->N == b->N, "gemm_case: the pair needs a.N == b.N (%lld, %lld)", (long long)a->N, (long long)b->N);
        const GemmPath p = resolve_gemm_pair(oa, ob);
        a->path = b->path = p.word();
        if (a->dry_run) return DAISY_OK;
        if (epi == EPI_STORE) run_gemm_pair<EPI_STORE>(oa, ob, p, s);
        else run_gemm_pair<EPI_ATOMIC>(oa, ob, p, s);
    } else if (a->launcher == DAISY_GEMM_LAUNCH_H) {
        const GemmPath p = resolve_gemm_h(oa, epi);
        a->path = p.word();
        if (a->dry_run) return DAISY_OK;
        if (epi == EPI_BIAS_RELU) run_gemm_h<EPI_BIAS_RELU>(oa, p, s);
        else if (epi == EPI_GATE) run_gemm_h<EPI_GATE>(oa, p, s);
        else run_gemm_h<EPI_ATOMIC>(oa, p, s);
    } else {
        const GemmPath p = resolve_gemm(oa, epi);
        a->path = p.word();
        if (a->dry_run) return DAISY_OK;
        if (epi == EPI_STORE) run_gemm<EPI_STORE>(oa, p, s);
        else if (epi == EPI_BIAS_RELU) run_gemm<EPI_BIAS_RELU>(oa, p, s);
        else if (epi == EPI_GATE) run_gemm<EPI_GATE>(oa, p, s);
        else run_gemm<EPI_ATOMIC>(oa, p, s);
    }
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // extern "C"
