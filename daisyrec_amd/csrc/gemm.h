// The MFMA products of the library (gemm.hip): C = A B^T-style contractions with arbitrary strides, in fp32, with bf16
// MFMA inputs, or over operands stored as bf16.  Internal: the exported entry points are daisy_gemm_* (daisyrec_amd.h).
#pragma once
#include "common.h"

namespace daisy {

constexpr int kGemmBM = 128;   // block tile rows (2 x 2 waves, each 64 rows)

enum { EPI_STORE = 0, EPI_BIAS_RELU = 1, EPI_GATE = 2, EPI_ATOMIC = 3 };

struct GemmOp {
    const float *A; int64_t sam, sak;     // A(m,k) = A[m*sam + k*sak]
    const float *B; int64_t sbn, sbk;     // B(n,k) = B[n*sbn + k*sbk]
    float *C; int64_t ldc, scn;           // C(m,n) = C[m*ldc + n*scn]   (scn = 0 means 1)
    int64_t M; int N; int64_t K;
    const float *bias;                    // EPI_BIAS_RELU
    const float *gate; int64_t ldg;       // EPI_GATE: out = acc * (gate(m,n) > 0 ? gate_scale : 0)
    float gate_scale;
    uint32_t drop_thresh, drop_stream;    // dropout on output element (m,n), idx = m*N + n; thresh 0: off
    float drop_scale;
    uint64_t drop_seed;
    int64_t k_chunk;                      // reduction range per blockIdx.z
    int64_t slice_stride;                 // EPI_ATOMIC: != 0 - slice z STORES its partial product at C + z * slice_stride
                                          // (summed in slice order by k_reduce_slices: reproducible); 0 - fp32 atomics into C
    int vec_a, vec_b;                     // set by launch_gemm: operand qualifies for the float4 path
    int bf16;                             // throughput mode: bf16-input MFMA where the tile shape allows it
    // bf16 STORAGE (precision level 2: activations and a copy of the weights live as bf16 in HBM): when A16 is set the
    // operands are read through A16 / B16 (same strides, in elements), the gate through G16, and the result goes to
    // C16 (EPI_BIAS_RELU / EPI_GATE) or, in fp32, to C (EPI_ATOMIC)
    const uint16_t *A16, *B16, *G16;
    uint16_t *C16;
};

// What a launcher decided for one GemmOp: the kernel instantiation and its grid.  resolve_gemm / resolve_gemm_h /
// resolve_gemm_pair (gemm.hip) fill it - and finish the op: k_chunk clamped to K, vec_a / vec_b set - before anything
// is launched; the launch step only reads it.  daisy_gemm_case reports word().
enum { GEMM_F32 = 0, GEMM_BF16IN = 1, GEMM_H = 2, GEMM_PAIR = 3 };
struct GemmPath {
    int family;                           // GEMM_*: k_gemm, k_gemm_bf16, k_gemm_h, k_gemm_pair
    int wn;                               // 32-column MFMA blocks per wave: 1 (64-column tiles) or 2 (128)
    bool fast, drop;                      // template arguments FAST (always set for k_gemm_bf16; k_gemm_h and the pair have none), DROP
    bool ak, bk;                          // k_gemm_h: operand A / B is contiguous along k
    unsigned gx, gy, splits;              // the grid; splits = k slices (pair: of the first product)
    unsigned ax, splits_b;                // pair: row tiles of the first product, k slices of the second
    // family | wn << 2 | fast << 4 | drop << 5 | ak << 6 | bk << 7 | splits << 8 | splits_b << 20  (12 bits per slice count)
    uint32_t word() const {
        return (uint32_t)family | (uint32_t)wn << 2 | (uint32_t)fast << 4 | (uint32_t)drop << 5 | (uint32_t)ak << 6 |
               (uint32_t)bk << 7 | (splits & 0xFFFu) << 8 | (splits_b & 0xFFFu) << 20;
    }
};
GemmPath resolve_gemm(GemmOp &op, int epi);
GemmPath resolve_gemm_h(GemmOp &op, int epi);
GemmPath resolve_gemm_pair(GemmOp &a, GemmOp &b);

// The launchers exist for the epilogues their callers use (instantiated in gemm.hip; another one is a link error):
//   launch_gemm       STORE, BIAS_RELU, GATE, ATOMIC: fp32 storage (op.bf16: bf16 MFMA inputs where the shape allows it)
//   launch_gemm_h     BIAS_RELU, GATE, ATOMIC: bf16 storage, only for shapes gemm_h_ok accepts
//   launch_gemm_pair  STORE, ATOMIC: two products of the same (N, tile width) in one launch
template <int EPI> void launch_gemm(GemmOp op, hipStream_t s);
template <int EPI> void launch_gemm_h(GemmOp op, hipStream_t s);
template <int EPI> void launch_gemm_pair(GemmOp a, GemmOp b, hipStream_t s);

// shapes the bf16-storage kernel takes: whole tiles, k ranges in multiples of 32, 16-byte aligned rows
bool gemm_h_ok(const GemmOp &op);

// fp32 -> bf16 (round to nearest even) of a [n / cols][cols] matrix, as stored (y) and transposed (yt)
void to_bf16_and_transpose(const float *x, int64_t n, int cols, uint16_t *y, uint16_t *yt, hipStream_t s);

// ---- the fp32 MFMA product (k_gemm): C(m,n) = sum_k A(m,k) B(n,k) with
// A(m,k) = A[m*sam + k*sak], B(n,k) = B[n*sbn + k*sbk], C(m,n) = C[m*ldc + n].  k_chunk >= K: C is written;
// k_chunk < K: slice z of the k range [z*k_chunk, (z+1)*k_chunk) STORES its partial product at C + z*slice_stride
// (slice_stride != 0; the caller sums the slices in a fixed order).
void gemm_f32(const float *A, int64_t sam, int64_t sak, const float *B, int64_t sbn, int64_t sbk, float *C, int64_t ldc,
              int64_t M, int N, int64_t K, int64_t k_chunk, int64_t slice_stride, hipStream_t s);

}  // namespace daisy
