// NeuMF (daisy/model/NeuMFRecommender.py) on gfx950.
//
//   forward   k_nmf_gather      x0 = [uM[u] | iM[item]] (dropout of layer 1 applied), g = uG[u]*iG[item],
//                               regulariser sums of the gathered rows (training only)
//             launch_gemm<EPI_BIAS_RELU>   x_l = ReLU(x_{l-1} W_l^T + b_l) (* dropout mask of layer l+1): the MFMA
//                               products of gemm.hip
//             k_nmf_predict     pred = <Wp, [g | x_L]> + bp
//   loss      k_nmf_loss        criterion epilogue shared with MF (pair_coef) -> d loss / d pred
//             k_nmf_finalize    norms + NeuMF.calc_loss value
//   backward  k_nmf_pred_bwd    dZ_L = dpred * Wp[mlp part] gated by x_L > 0;  gWp, gbp
//             launch_gemm<EPI_ATOMIC>   gW_l = dZ_l^T x_{l-1}: split-K slices side by side, added in order (k_reduce_slices)
//             k_colsum          gb_l += column sums of dZ_l
//             launch_gemm<EPI_GATE>     dZ_{l-1} = (dZ_l W_l) gated by x_{l-1} > 0 (layer 1: dropout mask of x0)
//             neumf_scatter     embedding gradients by table-row owners (no atomics) + the regulariser gradients
//                               exactly as NeuMFRecommender.py:149-167 lists them: csrc/neumf_scatter.hip
// Which of these a call runs - and which of them the fused kernels of csrc/neumf_mid.hip and csrc/neumf_tower.hip replace -
// is decided once per call: neumf_path.
// Dropout: x_{l-1} is stored already masked and scaled, so "x > 0" carries mask and ReLU gate at once.
#include <stdlib.h>

#include "common.h"
#include "gemm.h"
#include "mfma.h"
#include "neumf_internal.h"
#include "pairs.h"

namespace daisy {

// ---------------------------------------------------------------------------------------------
// the three pair layouts of daisy_neumf_scores plus the training batch
// ---------------------------------------------------------------------------------------------

struct L16 { static constexpr int LPR = 16; };

// x0[r] = [uM[user] | iM[item]] (* dropout), g[r] = uG[user]*iG[item]; TRAIN: the ten regulariser sums.
// H: the activations live as bf16 in HBM (precision level 2)
// FACT (round 5, "the first layer through the tables"): the MLP's first layer is linear in the concatenated embedding
// rows, z1[r] = W1[:, :dm] uM[user] + W1[:, dm:] iM[item] + b1, and a step of R rows meets only U + I DISTINCT table rows
// (ml-1m: 9746 against 524 288).  So T_u = uM W1[:, :dm]^T and T_i = iM W1[:, dm:]^T are two small GEMMs over the tables
// (Fact::tu, Fact::ti: fp32 [rows][n1]) and x1[r] = relu(T_u[user] + T_i[item] + b1) is a gather: x0 - 1 KB per row in bf16 -
// is never formed, the largest GEMM of the tower and its 2 x 512-column operand stream are gone.  The backward pass
// mirrors it (neumf_first_layer_bwd).  Needs dropout = 0 (a mask on x0's elements would not factor).
struct Fact {
    const uint16_t *tu, *ti; const float *b1; uint16_t *x1; int n1; const float2 *nu, *ni;     // nu / ni: k_nmf_row_norms
    const float *tu32, *ti32; float *x1_32;      // round 6, the fp32 (parity) mode: the products and x1 stay fp32
};
// (the products are handed to the gather as bf16: it is bound by reading them - 2 x 1 KB per row in fp32 from beyond L2 -
// and the plain path rounds x0 and W1 to bf16 BEFORE the product)
__global__ void k_f32_to_bf16(const float *__restrict__ x, int64_t n, uint16_t *__restrict__ y) {
    for (int64_t e = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) * 2; e < n; e += (int64_t)gridDim.x * blockDim.x * 2)
        *reinterpret_cast<uint32_t *>(y + e) = bf16_pack2(x[e], x[e + 1]);
}

template <bool TRAIN, bool H = false, bool FACT = false>
__global__ __launch_bounds__(kBlock) void k_nmf_gather(daisy_neumf_params p, PairSrc src, int64_t R, int d,
                                                       int dm, int pointwise, float *__restrict__ X0,
                                                       float *__restrict__ G, uint32_t thresh,
                                                       float scale, uint64_t seed,
                                                       double *__restrict__ stats, Fact fact = Fact{}) {
    const int lane = threadIdx.x % 16, group = threadIdx.x / 16;
    const int64_t gstride = (int64_t)gridDim.x * (kBlock / 16);
    float s1[5] = {0, 0, 0, 0, 0}, s2[5] = {0, 0, 0, 0, 0};
    for (int64_t r = (int64_t)blockIdx.x * (kBlock / 16) + group; r < R; r += gstride) {
        int64_t user, item;
        pair_ids(src, r, user, item);
        const bool first = !TRAIN || r < src.B;            // rows r >= B repeat the users with the negatives
        // a lane takes 4 consecutive columns: 16-byte table reads, 16-byte (fp32) or 8-byte (bf16) stores - the
        // first version moved one element per lane and stored bf16 two bytes at a time (363 us per 524 288 rows)
        const float *um = p.uM + user * dm, *im = p.iM + item * dm;
        float *x = X0 + r * (int64_t)(2 * dm);
        uint16_t *xh = reinterpret_cast<uint16_t *>(X0) + r * (int64_t)(2 * dm);
        if constexpr (FACT && !H) {
            // fp32 mode: x1 = relu((T_u[user] + T_i[item]) + b1) in fp32 - the reference's first layer up to the association of
            // its 2 dm-term dot product (two dm-term products, then two adds)
            const float *tu = fact.tu32 + user * fact.n1, *ti = fact.ti32 + item * fact.n1;
            float *x1 = fact.x1_32 + r * (int64_t)fact.n1;
            for (int c = 4 * lane; c < fact.n1; c += 64) {
                const float4 a4 = *reinterpret_cast<const float4 *>(tu + c), b4 = *reinterpret_cast<const float4 *>(ti + c);
                const float4 c4 = *reinterpret_cast<const float4 *>(fact.b1 + c);
                *reinterpret_cast<float4 *>(x1 + c) = make_float4(fmaxf((a4.x + b4.x) + c4.x, 0.f), fmaxf((a4.y + b4.y) + c4.y, 0.f),
                                                                  fmaxf((a4.z + b4.z) + c4.z, 0.f), fmaxf((a4.w + b4.w) + c4.w, 0.f));
            }
        }
        if constexpr (FACT && H) {
            // x1 from the two table products; the embedding rows themselves are read only where the regulariser counts
            // them (the positive half of the rows: NeuMFRecommender.py:149-167)
            const uint16_t *tu = fact.tu + user * fact.n1, *ti = fact.ti + item * fact.n1;
            uint16_t *x1 = fact.x1 + r * (int64_t)fact.n1;
            for (int c = 4 * lane; c < fact.n1; c += 64) {
                const uint2 ah = *reinterpret_cast<const uint2 *>(tu + c), bh = *reinterpret_cast<const uint2 *>(ti + c);
                const float4 a4 = make_float4(__uint_as_float(ah.x << 16), __uint_as_float(ah.x & 0xFFFF0000u),
                                              __uint_as_float(ah.y << 16), __uint_as_float(ah.y & 0xFFFF0000u));
                const float4 b4 = make_float4(__uint_as_float(bh.x << 16), __uint_as_float(bh.x & 0xFFFF0000u),
                                              __uint_as_float(bh.y << 16), __uint_as_float(bh.y & 0xFFFF0000u));
                const float4 c4 = *reinterpret_cast<const float4 *>(fact.b1 + c);
                const float z0 = fmaxf((a4.x + b4.x) + c4.x, 0.f), z1 = fmaxf((a4.y + b4.y) + c4.y, 0.f);
                const float z2 = fmaxf((a4.z + b4.z) + c4.z, 0.f), z3 = fmaxf((a4.w + b4.w) + c4.w, 0.f);
                *reinterpret_cast<uint2 *>(x1 + c) = make_uint2(bf16_pack2(z0, z1), bf16_pack2(z2, z3));
            }
        }
        if constexpr (FACT && TRAIN) {
            if (first && lane == 0) {              // the MLP rows' share of the regulariser sums, from the per-row table
                const float2 a = fact.nu[user], b = fact.ni[item];
                s1[1] += a.x; s2[1] += a.y; s1[3] += b.x; s2[3] += b.y;
            }
        }
        for (int c = 4 * lane; c < dm && !FACT; c += 64) {
            const float4 a4 = *reinterpret_cast<const float4 *>(um + c), b4 = *reinterpret_cast<const float4 *>(im + c);
            float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
            if (TRAIN) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (first) {
                        s1[1] += fabsf(a[k]); s2[1] = fmaf(a[k], a[k], s2[1]);
                        s1[3] += fabsf(b[k]); s2[3] = fmaf(b[k], b[k], s2[3]);
                    }
                    if (thresh) {
                        a[k] = drop_keep(seed, 1, (uint64_t)r * (2 * dm) + c + k, thresh) ? a[k] * scale : 0.f;
                        b[k] = drop_keep(seed, 1, (uint64_t)r * (2 * dm) + dm + c + k, thresh) ? b[k] * scale : 0.f;
                    }
                }
            }
            if constexpr (FACT) {
                // (no x0)
            } else if constexpr (H) {
                *reinterpret_cast<uint2 *>(xh + c) =
                    make_uint2(bf16_pack2(a[0], a[1]), bf16_pack2(a[2], a[3]));
                *reinterpret_cast<uint2 *>(xh + dm + c) =
                    make_uint2(bf16_pack2(b[0], b[1]), bf16_pack2(b[2], b[3]));
            } else {
                *reinterpret_cast<float4 *>(x + c) = make_float4(a[0], a[1], a[2], a[3]);
                *reinterpret_cast<float4 *>(x + dm + c) = make_float4(b[0], b[1], b[2], b[3]);
            }
        }
        const float *ug = p.uG + user * d, *ig = p.iG + item * d;
        for (int c = 4 * lane; c < d; c += 64) {
            const float4 a4 = *reinterpret_cast<const float4 *>(ug + c), b4 = *reinterpret_cast<const float4 *>(ig + c);
            const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
            *reinterpret_cast<float4 *>(G + r * (int64_t)d + c) = make_float4(a[0] * b[0], a[1] * b[1], a[2] * b[2], a[3] * b[3]);
            if (TRAIN) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (first) { s1[0] += fabsf(a[k]); s2[0] = fmaf(a[k], a[k], s2[0]); s1[2] += fabsf(b[k]); s2[2] = fmaf(b[k], b[k], s2[2]); }
                    else if (!pointwise) { s1[4] += fabsf(b[k]); s2[4] = fmaf(b[k], b[k], s2[4]); }
                }
            }
        }
    }
    if constexpr (TRAIN) {
        __shared__ double sm[kBlock / kWave][10];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const double a = wave_sum_f64((double)s1[k]), b = wave_sum_f64((double)s2[k]);
            if (threadIdx.x % kWave == 0) { sm[threadIdx.x / kWave][k] = a; sm[threadIdx.x / kWave][5 + k] = b; }
        }
        __syncthreads();
        if (threadIdx.x < 10) {
            double t = 0.0;
            for (int w = 0; w < kBlock / kWave; ++w) t += sm[w][threadIdx.x];
            atomicAdd(stats + DAISY_NST_L1 + threadIdx.x, t);        // L1[5] then SQ[5] are adjacent
        }
    }
}

// pred[r] = <Wp[:dg], g[r]> + <Wp[dg:], x_L[r]> + bp      (dg = 0 for model MLP, nl = 0 for model GMF)
template <bool H = false>
__global__ __launch_bounds__(kBlock) void k_nmf_predict(const float *__restrict__ G, int dg,
                                                        const float *__restrict__ XL, int nl,
                                                        const float *__restrict__ Wp,
                                                        const float *__restrict__ bp, int64_t R,
                                                        float *__restrict__ pred) {
    const int lane = threadIdx.x % 16, group = threadIdx.x / 16;
    const int64_t gstride = (int64_t)gridDim.x * (kBlock / 16);
    for (int64_t r = (int64_t)blockIdx.x * (kBlock / 16) + group; r < R; r += gstride) {
        float s = 0.f;
        for (int c = lane; c < dg; c += 16) s = fmaf(Wp[c], G[r * (int64_t)dg + c], s);
        for (int c = lane; c < nl; c += 16) {
            float x;
            if constexpr (H) x = bf16_to_f32(reinterpret_cast<const uint16_t *>(XL)[r * (int64_t)nl + c]);
            else x = XL[r * (int64_t)nl + c];
            s = fmaf(Wp[dg + c], x, s);
        }
        s = group_sum<L16>(s);
        if (lane == 0) pred[r] = s + bp[0];
    }
}

// criterion epilogue (AbstractRecommender.py:79-93, daisy/utils/loss.py): d loss / d pred for both rows of a sample
__global__ __launch_bounds__(kBlock) void k_nmf_loss(const float *__restrict__ pred,
                                                     const int32_t *__restrict__ j, int64_t B,
                                                     int loss_type, float gamma, int pointwise,
                                                     float *__restrict__ dpred,
                                                     double *__restrict__ stats,
                                                     float *__restrict__ gbp_ws) {
    // gbp = sum_b (cp_b + cn_b), paired per sample: under BPR / HL every pair is exactly 0, as it is in
    // the reference's autograd (a rounding residue here would be blown up to +-lr by Adam)
    double acc = 0.0;
    float accb = 0.f;
    for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < B; b += (int64_t)gridDim.x * blockDim.x) {
        float term, cp, cn;
        pair_coef(loss_type, pred[b], pointwise ? (float)j[b] : pred[B + b], gamma, term, cp, cn);
        dpred[b] = cp;
        if (!pointwise) dpred[B + b] = cn;
        acc += (double)term;
        accb += cp + cn;
    }
    acc = wave_sum_f64(acc);
    const double sb = wave_sum_f64((double)accb);
    __shared__ double smb[kBlock / kWave];
    if (threadIdx.x % kWave == 0) {
        atomicAdd(stats + DAISY_NST_LOSS_DATA, acc);
        smb[threadIdx.x / kWave] = sb;
    }
    __syncthreads();
    if (threadIdx.x == 0) {                            // waves in order; the workgroups' sums are added by k_reduce_slices
        double t = 0.0;
        for (int w = 0; w < kBlock / kWave; ++w) t += smb[w];
        gbp_ws[blockIdx.x] = (float)t;
    }
}

// NeuMFRecommender.py:149-167 summed up: the negative item's GMF rows enter twice, its MLP rows never
__global__ void k_nmf_finalize(double *__restrict__ stats, float reg_1, float reg_2, int pointwise) {
    if (threadIdx.x || blockIdx.x) return;
    double l1 = 0.0, fro = 0.0;
    for (int k = 0; k < 5; ++k) {
        const double n = sqrt(stats[DAISY_NST_SQ + k]);
        stats[DAISY_NST_NORM + k] = n;
        const double w = (k == 4) ? (pointwise ? 0.0 : 2.0) : 1.0;
        l1 += w * stats[DAISY_NST_L1 + k];
        fro += w * n;
    }
    const double loss = stats[DAISY_NST_LOSS_DATA] + (double)reg_1 * l1 + (double)reg_2 * fro;
    stats[DAISY_NST_LOSS] = loss;
    stats[DAISY_NST_LOSS_SUM] += loss;
}

// out[c] += sum_s ws[s][c], s = 0 .. nslices-1 in that order: the second half of every reduction over the batch rows
// whose first half is spread over workgroups (split-K slices of the weight-gradient GEMMs, row tiles of the column
// sums, workgroups of the predict layer's backward pass).  Fixed order instead of fp32 atomics: two runs of a step
// give the same bits.
__global__ __launch_bounds__(kBlock) void k_reduce_slices(const float *__restrict__ ws, int nslices, int64_t len,
                                                          float *__restrict__ out) {
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < len; c += (int64_t)gridDim.x * blockDim.x) {
        float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
        int sidx = 0;
        for (; sidx + 3 < nslices; sidx += 4) {                          // four loads in flight, fixed association
            t0 += ws[(int64_t)sidx * len + c];
            t1 += ws[(int64_t)(sidx + 1) * len + c];
            t2 += ws[(int64_t)(sidx + 2) * len + c];
            t3 += ws[(int64_t)(sidx + 3) * len + c];
        }
        for (; sidx < nslices; ++sidx) t0 += ws[(int64_t)sidx * len + c];
        out[c] += (t0 + t1) + (t2 + t3);
    }
}

// the same into a [rows][cols] block of a wider matrix (leading dimension ldo): slices are contiguous [rows][cols]
__global__ __launch_bounds__(kBlock) void k_reduce_slices_2d(const float *__restrict__ ws, int nslices, int rows, int cols,
                                                             float *__restrict__ out, int64_t ldo,
                                                             const float *__restrict__ ws_b = nullptr, int nslices_b = 0,
                                                             float *__restrict__ out_b = nullptr) {
    if (blockIdx.y) { ws = ws_b; nslices = nslices_b; out = out_b; }      // (a second block of the same shape in the same launch)
    const int64_t len = (int64_t)rows * cols;
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < len; c += (int64_t)gridDim.x * blockDim.x) {
        float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
        int sidx = 0;
        for (; sidx + 3 < nslices; sidx += 4) {
            t0 += ws[(int64_t)sidx * len + c];
            t1 += ws[(int64_t)(sidx + 1) * len + c];
            t2 += ws[(int64_t)(sidx + 2) * len + c];
            t3 += ws[(int64_t)(sidx + 3) * len + c];
        }
        for (; sidx < nslices; ++sidx) t0 += ws[(int64_t)sidx * len + c];
        out[(c / cols) * ldo + (c % cols)] += (t0 + t1) + (t2 + t3);
    }
}

// per table row: (sum |x|, sum x^2) - what the regulariser sums of a step need from an MLP embedding row
// (k_nmf_gather<FACT>, which does not read the rows themselves)
__global__ __launch_bounds__(kBlock) void k_nmf_row_norms(const float *__restrict__ Ta, int64_t rows_a, const float *__restrict__ Tb,
                                                          int64_t rows_b, int width, float2 *__restrict__ out_a,
                                                          float2 *__restrict__ out_b) {
    // (both tables in one launch: blockIdx.y)
    const float *__restrict__ T = blockIdx.y ? Tb : Ta;
    const int64_t rows = blockIdx.y ? rows_b : rows_a;
    float2 *__restrict__ out = blockIdx.y ? out_b : out_a;
    const int lane = threadIdx.x % 16, group = threadIdx.x / 16;
    const int64_t gstride = (int64_t)gridDim.x * (kBlock / 16);
    for (int64_t r = (int64_t)blockIdx.x * (kBlock / 16) + group; r < rows; r += gstride) {
        float a = 0.f, b = 0.f;
        for (int c = 4 * lane; c < width; c += 64) {
            const float4 v = *reinterpret_cast<const float4 *>(T + r * (int64_t)width + c);
            a += (fabsf(v.x) + fabsf(v.y)) + (fabsf(v.z) + fabsf(v.w));
            b = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, b))));
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) { a += __shfl_xor(a, o, 16); b += __shfl_xor(b, o, 16); }
        if (lane == 0) out[r] = make_float2(a, b);
    }
}

// dZ_L[r] = dpred[r] * Wp[dg:] gated by x_L[r] > 0;  gWp += sum_r dpred[r]*[g[r] | x_L[r]];  gbp += sum dpred
// (the column sums leave as one row of `ws` per workgroup: ws[blockIdx.x][dg + nl], summed by k_reduce_slices)
template <bool H = false>
__global__ __launch_bounds__(kBlock) void k_nmf_pred_bwd(const float *__restrict__ dpred,
                                                         const float *__restrict__ G, int dg,
                                                         const float *__restrict__ XL, int nl,
                                                         const float *__restrict__ Wp, int64_t R,
                                                         float *__restrict__ DZ, float *__restrict__ ws) {
    __shared__ float colg[kBlock / 16][128];         // one sweep of 128 columns: every lane group's partial sums
    const int lane = threadIdx.x % 16, group = threadIdx.x / 16;
    const int64_t gstride = (int64_t)gridDim.x * (kBlock / 16);
    for (int c0 = 0; c0 < dg + nl; c0 += 16 * 8) {   // 8 column registers per lane per sweep
        float part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int64_t r = (int64_t)blockIdx.x * (kBlock / 16) + group; r < R; r += gstride) {
            const float dp = dpred[r];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int c = c0 + q * 16 + lane;
                if (c < dg) part[q] = fmaf(dp, G[r * (int64_t)dg + c], part[q]);
                else if (c < dg + nl) {
                    float x;
                    if constexpr (H) x = bf16_to_f32(reinterpret_cast<const uint16_t *>(XL)[r * (int64_t)nl + (c - dg)]);
                    else x = XL[r * (int64_t)nl + (c - dg)];
                    part[q] = fmaf(dp, x, part[q]);
                    const float dzv = (x > 0.f) ? dp * Wp[c] : 0.f;
                    if constexpr (H) reinterpret_cast<uint16_t *>(DZ)[r * (int64_t)nl + (c - dg)] = (uint16_t)bf16_rne(dzv);
                    else DZ[r * (int64_t)nl + (c - dg)] = dzv;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) colg[group][q * 16 + lane] = part[q];
        __syncthreads();
        if ((int)threadIdx.x < 128 && c0 + (int)threadIdx.x < dg + nl) {           // groups in order
            float t = 0.f;
#pragma unroll
            for (int gq = 0; gq < kBlock / 16; ++gq) t += colg[gq][threadIdx.x];
            ws[(int64_t)blockIdx.x * (dg + nl) + c0 + threadIdx.x] = t;
        }
        __syncthreads();
    }
}

// the same for dg == nl == d <= 64, d % 4 == 0 (every NeuMF tower: the last layer is `factors` wide like the GMF
// product): 16 lanes per row, each lane 4 consecutive columns of g[r] and of x_L[r] with one vector load each
template <bool H>
__global__ __launch_bounds__(kBlock) void k_nmf_pred_bwd_v(const float *__restrict__ dpred,
                                                           const float *__restrict__ G, int d,
                                                           const float *__restrict__ XL,
                                                           const float *__restrict__ Wp, int64_t R,
                                                           float *__restrict__ DZ, float *__restrict__ ws) {
    __shared__ float colg[kBlock / 16][128];          // [lane group][g columns 0..63 | x columns 64..127]
    const int lane = threadIdx.x % 16, group = threadIdx.x / 16;
    const bool on = 4 * lane < d;
    const int c4 = on ? 4 * lane : 0;
    const int64_t gstride = (int64_t)gridDim.x * (kBlock / 16);
    const float4 wp = *reinterpret_cast<const float4 *>(Wp + d + c4);
    float pg[4] = {0.f, 0.f, 0.f, 0.f}, px[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t r = (int64_t)blockIdx.x * (kBlock / 16) + group; r < R; r += gstride) {
        const float dp = dpred[r];
        const float4 g4 = *reinterpret_cast<const float4 *>(G + r * d + c4);
        float x[4];
        if constexpr (H) {
            const uint2 q = *reinterpret_cast<const uint2 *>(reinterpret_cast<const uint16_t *>(XL) + r * d + c4);
            x[0] = __uint_as_float(q.x << 16); x[1] = __uint_as_float(q.x & 0xFFFF0000u);
            x[2] = __uint_as_float(q.y << 16); x[3] = __uint_as_float(q.y & 0xFFFF0000u);
        } else {
            const float4 q = *reinterpret_cast<const float4 *>(XL + r * d + c4);
            x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
        }
        pg[0] = fmaf(dp, g4.x, pg[0]); pg[1] = fmaf(dp, g4.y, pg[1]);
        pg[2] = fmaf(dp, g4.z, pg[2]); pg[3] = fmaf(dp, g4.w, pg[3]);
        const float w4[4] = {wp.x, wp.y, wp.z, wp.w};
        float dz[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            px[k] = fmaf(dp, x[k], px[k]);
            dz[k] = (x[k] > 0.f) ? dp * w4[k] : 0.f;
        }
        if (on) {
            if constexpr (H)
                *reinterpret_cast<uint2 *>(reinterpret_cast<uint16_t *>(DZ) + r * d + c4) =
                    make_uint2(bf16_pack2(dz[0], dz[1]), bf16_pack2(dz[2], dz[3]));
            else
                *reinterpret_cast<float4 *>(DZ + r * d + c4) = make_float4(dz[0], dz[1], dz[2], dz[3]);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { colg[group][4 * lane + k] = on ? pg[k] : 0.f; colg[group][64 + 4 * lane + k] = on ? px[k] : 0.f; }
    __syncthreads();
    const int t = (int)threadIdx.x;
    if (t < 128) {                                    // lane groups in order; ws row = [g columns (d) | x columns (d)]
        float acc = 0.f;
#pragma unroll
        for (int gq = 0; gq < kBlock / 16; ++gq) acc += colg[gq][t];
        if (t < d) ws[(int64_t)blockIdx.x * (2 * d) + t] = acc;
        else if (t >= 64 && t < 64 + d) ws[(int64_t)blockIdx.x * (2 * d) + d + (t - 64)] = acc;
    }
}

// ws[row tile][n] = sum over the tile's rows of X[r*ld + n]: a block takes 64 columns x kColsumRows rows (grid = column
// tiles x row tiles); k_reduce_slices adds the row tiles in order
constexpr int kColsumRows = 512;
// rows per workgroup: 512, or 64 for matrices of a few thousand rows (a step of 512 rows was ONE workgroup per 64 columns
// walking all of them: 15 us for 100 KB)
static inline int colsum_rows(int64_t R) { return R <= 8192 ? 64 : kColsumRows; }
template <bool H = false>
__global__ __launch_bounds__(kBlock) void k_colsum(const float *__restrict__ X, int64_t R, int N, int64_t ld,
                                                   float *__restrict__ out, int rows_per_block = kColsumRows) {
    auto at = [&](int64_t idx) -> float {
        if constexpr (H) return bf16_to_f32(reinterpret_cast<const uint16_t *>(X)[idx]);
        else return X[idx];
    };
    __shared__ float sm[4][64];
    const int c = threadIdx.x % 64, rr = threadIdx.x / 64;
    const int n = blockIdx.x * 64 + c;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
    const int64_t r1 = (r0 + rows_per_block < R) ? r0 + rows_per_block : R;
    float s0 = 0.f, s1 = 0.f;
    if (n < N) {
        int64_t r = r0 + rr;
        for (; r + 4 < r1; r += 8) { s0 += at(r * ld + n); s1 += at((r + 4) * ld + n); }
        if (r < r1) s0 += at(r * ld + n);
    }
    sm[rr][c] = s0 + s1;
    __syncthreads();
    if (rr == 0 && n < N) out[(int64_t)blockIdx.y * N + n] = (sm[0][c] + sm[1][c]) + (sm[2][c] + sm[3][c]);
}

// the same for a bf16 matrix whose rows are whole 16-byte vectors (N % 8 == 0, N <= 2048, ld == N): a thread owns
// 8 consecutive columns and reads them with one 16-byte load per row; a block takes kColsumRowsH rows
constexpr int kColsumRowsH = 512;
__global__ __launch_bounds__(kBlock) void k_colsum_h(const uint16_t *__restrict__ X, int64_t R, int N,
                                                     float *__restrict__ out) {
    __shared__ float sm[kBlock][9];
    const int vpr = N / 8;                            // vectors per row (a divisor of kBlock or a multiple: see the launch)
    const int cv = threadIdx.x % vpr, rr = threadIdx.x / vpr, rpp = kBlock / vpr;
    const int64_t r0 = (int64_t)blockIdx.x * kColsumRowsH;
    const int64_t r1 = (r0 + kColsumRowsH < R) ? r0 + kColsumRowsH : R;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto add = [&](const uint4 &q) {
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            acc[2 * k] += __uint_as_float(w[k] << 16);
            acc[2 * k + 1] += __uint_as_float(w[k] & 0xFFFF0000u);
        }
    };
    const uint16_t *col = X + cv * 8;
    int64_t r = r0 + rr;
    for (; r + 3 * rpp < r1; r += 4 * rpp) {          // four rows in flight per thread
        const uint4 q0 = *reinterpret_cast<const uint4 *>(col + r * N);
        const uint4 q1 = *reinterpret_cast<const uint4 *>(col + (r + rpp) * N);
        const uint4 q2 = *reinterpret_cast<const uint4 *>(col + (r + 2 * rpp) * N);
        const uint4 q3 = *reinterpret_cast<const uint4 *>(col + (r + 3 * rpp) * N);
        add(q0); add(q1); add(q2); add(q3);
    }
    for (; r < r1; r += rpp) add(*reinterpret_cast<const uint4 *>(col + r * N));
#pragma unroll
    for (int k = 0; k < 8; ++k) sm[threadIdx.x][k] = acc[k];
    __syncthreads();
    for (int c = threadIdx.x; c < N; c += kBlock) {   // column c: vector c/8, element c%8, summed over the row groups
        float t = 0.f;
        for (int g = 0; g < rpp; ++g) t += sm[g * vpr + c / 8][c % 8];
        out[(int64_t)blockIdx.x * N + c] = t;          // (row tile blockIdx.x of the workspace: see k_colsum)
    }
}

}  // namespace daisy

using namespace daisy;

struct daisy_neumf_ctx {
    int64_t max_rows, U, I;
    int d, L, dm, model;
    int width[DAISY_NEUMF_MAX_LAYERS + 1];   // width[0] = 2*dm, width[l] = width[l-1]/2
    DeviceArena arena;
    float *X[DAISY_NEUMF_MAX_LAYERS + 1];    // X[0] = (dropped) concat input, X[l] = layer outputs
    float *G, *pred, *dpred, *DZ[2];
    uint16_t *W16[DAISY_NEUMF_MAX_LAYERS];   // bf16 copies of the MLP weights (precision level 2), refreshed per call
    uint16_t *W16T[DAISY_NEUMF_MAX_LAYERS];  // ... and their transposes [n_in][n_out]
    NeumfScatter scatter;                    // the embedding scatter's state (csrc/neumf_scatter.hip)
    int bf16;                                // daisy_neumf_ctx_set_precision: 0 fp32, 1 bf16 MFMA inputs, 2 bf16 storage
    // per-workgroup partial sums of the reductions over the batch rows (split-K slices of the weight-gradient GEMMs,
    // row tiles of the column sums ...), added in a fixed order by k_reduce_slices; allocated at the first training step
    float *det_ws;
    size_t det_ws_floats;
    float *fact_t;                           // T_u [U][n1] then T_i [I][n1]: the first layer through the tables (k_nmf_gather<FACT>)
    bool mid_fits;                           // k_nmf_mid: the layers fit the LDS (ctx_create)
};

constexpr int kWgradChunkDefault = 2048;
static int wgrad_chunk() {
    static const int v = getenv("DAISY_WGRAD_CHUNK") ? atoi(getenv("DAISY_WGRAD_CHUNK")) : kWgradChunkDefault;
    return v > 0 ? v : kWgradChunkDefault;
}

constexpr int kMidMaxRows = kScanMaxRows;   // steps k_nmf_mid takes (csrc/neumf_mid.hip): the ones its scatter, the scanning kernel, takes
static int neumf_need_det_ws(daisy_neumf_ctx *ctx) {
    if (ctx->det_ws) return DAISY_OK;
    const size_t splits = ((size_t)ctx->max_rows + wgrad_chunk() - 1) / wgrad_chunk();
    size_t layer = 1024;                               // (predict layer: <= 1024 workgroups x 512 columns, covered below)
    for (int l = 1; l <= ctx->L; ++l) {
        const size_t e = (size_t)ctx->width[l] * ctx->width[l - 1];
        if (e > layer) layer = e;
    }
    size_t n = splits * layer;
    const size_t pred = (size_t)1024 * 512;
    if (pred > n) n = pred;
    // the fused tower (csrc/neumf_tower.hip): one slab of partial sums per workgroup
    const size_t tower = (neumf_tower_ws_bytes(ctx->d, neumf_tower_blocks((ctx->max_rows + 63) / 64)) + 3) / 4;
    if (tower > n) n = tower;
    const int rows_mid = ctx->max_rows < kMidMaxRows ? (int)ctx->max_rows : kMidMaxRows;
    const size_t mid = (neumf_mid_ws_bytes(ctx->L, ctx->width, ctx->d, rows_mid) + 3) / 4;
    if (mid > n) n = mid;
    hipError_t e = hipMalloc((void **)&ctx->det_ws, n * sizeof(float));
    if (e != hipSuccess) {
        ctx->det_ws = nullptr;
        set_error("neumf: hipMalloc(%zu) for the reduction workspace failed: %s", n * sizeof(float), hipGetErrorString(e));
        return DAISY_ERR_HIP;
    }
    ctx->det_ws_floats = n;
    return DAISY_OK;
}

// Many slices (the split-K weight gradients: 256 slices of up to 131 072 elements; the column sums: 1024 slices of 64-256):
// one thread per element walking all slices left most of the chip idle with four loads in flight per thread - 33.5 MB in
// 66 us, and ONE workgroup for the column sums.  Here a workgroup takes C elements and its 256 / C thread groups every
// (256 / C)-th slice each; the partial sums meet in LDS in group order: still one fixed association per element.
template <int C>
__global__ __launch_bounds__(kBlock) void k_reduce_slices_wide(const float *__restrict__ ws, int nslices, int64_t len,
                                                               float *__restrict__ out) {
    constexpr int G = kBlock / C;
    __shared__ float sm[G][C];
    const int c = threadIdx.x % C, g = threadIdx.x / C;
    for (int64_t c0 = (int64_t)blockIdx.x * C; c0 < len; c0 += (int64_t)gridDim.x * C) {
        const int64_t col = c0 + c;
        float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
        if (col < len) {
            int sidx = g;
            for (; sidx + 3 * G < nslices; sidx += 4 * G) {
                t0 += ws[(int64_t)sidx * len + col];
                t1 += ws[(int64_t)(sidx + G) * len + col];
                t2 += ws[(int64_t)(sidx + 2 * G) * len + col];
                t3 += ws[(int64_t)(sidx + 3 * G) * len + col];
            }
            for (; sidx < nslices; sidx += G) t0 += ws[(int64_t)sidx * len + col];
        }
        sm[g][c] = (t0 + t1) + (t2 + t3);
        __syncthreads();
        if (g == 0 && col < len) {
            float t = sm[0][c];
#pragma unroll
            for (int k = 1; k < G; ++k) t += sm[k][c];
            out[col] += t;
        }
        __syncthreads();
    }
}

static void reduce_slices(const float *ws, int nslices, int64_t len, float *out, hipStream_t s) {
    if (nslices >= 32 && len >= 4096)
        hipLaunchKernelGGL((k_reduce_slices_wide<64>), dim3(grid_for(len, 64, 4096)), dim3(kBlock), 0, s, ws, nslices, len, out);
    else if (nslices >= 64)
        hipLaunchKernelGGL((k_reduce_slices_wide<16>), dim3(grid_for(len, 16, 4096)), dim3(kBlock), 0, s, ws, nslices, len, out);
    else
        hipLaunchKernelGGL(k_reduce_slices, dim3(grid_for(len, kBlock, 2048)), dim3(kBlock), 0, s, ws, nslices, len, out);
}

// What a call of R rows runs - the one place that decides, and that reads DAISY_NMF_MID / _FACT / _TOWER (per call: the tests
// switch them; each defaults to on, 0 keeps the layer-by-layer kernels for A/B and as the fused kernels' reference).
static NeumfPath neumf_path(const daisy_neumf_ctx *ctx, const daisy_neumf_params &p, int64_t R, bool train, uint32_t thresh) {
    auto on = [](const char *name) { const char *env = getenv(name); return !env || atoi(env) != 0; };
    const int L = ctx->L, model = ctx->model;
    NeumfPath q{};
    // precision level 2 applies when every GEMM of the call is made of whole tiles (else the call runs at level 1)
    q.H = ctx->bf16 == 2 && model != DAISY_NEUMF_GMF && R % kGemmBM == 0;
    for (int l = 0; l <= L; ++l)
        if (ctx->width[l] % 64 != 0) q.H = false;
    uintptr_t bits = (uintptr_t)p.Wp | (uintptr_t)p.uG | (uintptr_t)p.iG | (uintptr_t)p.uM | (uintptr_t)p.iM;
    for (int l = 0; l < L; ++l) bits |= (uintptr_t)p.W[l] | (uintptr_t)p.b[l];
    q.params_aligned = (bits & 15) == 0;
    q.w23_aligned = L >= 3 && (((uintptr_t)p.W[1] | (uintptr_t)p.W[2]) & 15) == 0;
    // small steps of the fp32 mode (the reference's own batch of 256 samples): everything between the gather and the scatter
    // in one launch with the layers' weights in LDS
    q.mid = on("DAISY_NMF_MID") && train && ctx->bf16 == 0 && model == DAISY_NEUMF_FULL && R <= kMidMaxRows && ctx->mid_fits &&
            q.params_aligned;
    // the first layer through the tables: training, no dropout, a first layer of the standard halving tower, fewer distinct
    // table rows than rows in the step, and not a step k_nmf_mid takes.  Bf16 storage (whole tiles) or the fp32 parity mode:
    // level 1 - bf16 MFMA inputs - keeps the plain path (its first layer rounds x0 and W1, which a product over the tables
    // would not)
    const bool mode_ok = (ctx->bf16 == 2) ? (q.H && ctx->dm % 64 == 0) : (ctx->bf16 == 0);
    q.fact = !q.mid && on("DAISY_NMF_FACT") && train && thresh == 0 && mode_ok && model != DAISY_NEUMF_GMF && L >= 1 &&
             ctx->width[1] == ctx->dm && ctx->U + ctx->I <= R;
    // the fused tower: bf16 storage behind the table products, the 4d -> 2d -> d tower at d = 64, the full model
    q.tower = on("DAISY_NMF_TOWER") && ctx->bf16 == 2 && q.fact && L == 3 && ctx->d == 64 && model == DAISY_NEUMF_FULL &&
              R % 64 == 0 && q.w23_aligned;
    return q;
}

static int neumf_need_fact(daisy_neumf_ctx *ctx) {
    if (ctx->fact_t) return DAISY_OK;
    // the products in fp32, the row norms (2 floats per row), the products again as bf16 (half a float per element)
    // (+ 32 floats: the bf16 copy starts on a 128-byte boundary - its rows are whole cache lines for the tower's gather)
    const size_t n = (size_t)(ctx->U + ctx->I) * ((size_t)ctx->width[1] + 2 + (size_t)ctx->width[1] / 2) + 32;
    if (hipMalloc((void **)&ctx->fact_t, n * sizeof(float)) != hipSuccess) {
        set_error("neumf: hipMalloc(%zu) of the first-layer table products failed", n * sizeof(float));
        ctx->fact_t = nullptr;
        return DAISY_ERR_HIP;
    }
    return DAISY_OK;
}

// x_L and pred for R pairs starting at src.base (eval: thresh == 0).  *fact (path.fact; null in eval): the table products
// as this call set them up, for the backward pass
static int neumf_forward_rows(daisy_neumf_ctx *ctx, const daisy_neumf_params *p, const NeumfPath &path, const PairSrc &src,
                              int64_t R, bool train, int pointwise, uint32_t thresh, float scale, uint64_t seed,
                              double *stats, Fact *fact, hipStream_t s) {
    const int d = ctx->d, dm = ctx->dm, L = ctx->L;
    const int grid = grid_for(R, kBlock / 16 * 2);
    const bool H = path.H;
    if (H) {          // bf16 copies of the MLP weights (a few hundred KB)
        // (the first layer's copy - the largest - has no reader when that layer runs through the tables, and there is none
        // at all under the fused tower, which rounds W2 / W3 as it loads them into LDS)
        for (int l = path.tower ? L + 1 : (path.fact ? 2 : 1); l <= L; ++l) {
            const int64_t nw = (int64_t)ctx->width[l] * ctx->width[l - 1];
            to_bf16_and_transpose(p->W[l - 1], nw, ctx->width[l - 1], ctx->W16[l - 1], ctx->W16T[l - 1], s);
        }
    }
    if (path.mid) return DAISY_OK;     // (the gather, the layers and the predict layer happen in k_nmf_mid)
    if (path.fact) {
        int rc = neumf_need_fact(ctx);
        if (rc) return rc;
        const int n1 = ctx->width[1];
        float *tu = ctx->fact_t, *ti = ctx->fact_t + (size_t)ctx->U * n1;
        GemmOp top[2];
        for (int side = 0; side < 2; ++side) {          // T = table x W1[:, half]^T  (fp32: the tables are fp32)
            GemmOp op{};
            op.A = side ? p->iM : p->uM; op.sam = dm; op.sak = 1;
            op.B = p->W[0] + (side ? dm : 0); op.sbn = ctx->width[0]; op.sbk = 1;
            op.C = side ? ti : tu; op.ldc = n1;
            op.M = side ? ctx->I : ctx->U; op.N = n1; op.K = dm;
            op.k_chunk = op.K;
            // fp32 products of the fp32 tables and weights, rounded to bf16 once (k_f32_to_bf16): the rounding points do not
            // depend on whether the table's row count happens to tile (oracle/neumf_numpy.py: neumf_grad_bf16 'fact')
            op.bf16 = 0;
            top[side] = op;
        }
        launch_gemm_pair<EPI_STORE>(top[0], top[1], s);      // (both sides in one launch: k_gemm_pair)
        float2 *nu = reinterpret_cast<float2 *>(ctx->fact_t + (size_t)(ctx->U + ctx->I) * n1), *ni = nu + ctx->U;
        hipLaunchKernelGGL(k_nmf_row_norms, dim3(grid_for(ctx->U > ctx->I ? ctx->U : ctx->I, kBlock / 16), 2), dim3(kBlock), 0, s, p->uM,
                           ctx->U, p->iM, ctx->I, dm, nu, ni);
        uint16_t *t16 = reinterpret_cast<uint16_t *>(ctx->fact_t + (((size_t)(ctx->U + ctx->I) * ((size_t)n1 + 2) + 31) / 32) * 32);
        const int64_t nt = (int64_t)(ctx->U + ctx->I) * n1;
        if (H) hipLaunchKernelGGL(k_f32_to_bf16, dim3(grid_for(nt, kBlock * 2)), dim3(kBlock), 0, s, tu, nt, t16);
        const Fact f{t16, t16 + (size_t)ctx->U * n1, p->b[0], reinterpret_cast<uint16_t *>(ctx->X[1]), n1, nu, ni, tu, ti, ctx->X[1]};
        *fact = f;
        if (path.tower) {        // the gather, the layers and the predict layer happen in the tower kernel
            DAISY_LAUNCH_CHECK();
            return DAISY_OK;
        }
        if (H) hipLaunchKernelGGL((k_nmf_gather<true, true, true>), dim3(grid), dim3(kBlock), 0, s, *p, src, R, d, dm, pointwise,
                                  ctx->X[0], ctx->G, thresh, scale, seed, stats, f);
        else hipLaunchKernelGGL((k_nmf_gather<true, false, true>), dim3(grid), dim3(kBlock), 0, s, *p, src, R, d, dm, pointwise,
                                ctx->X[0], ctx->G, thresh, scale, seed, stats, f);
    } else if (train) {
        if (H) hipLaunchKernelGGL((k_nmf_gather<true, true>), dim3(grid), dim3(kBlock), 0, s, *p, src, R, d, dm, pointwise,
                                  ctx->X[0], ctx->G, thresh, scale, seed, stats);
        else hipLaunchKernelGGL((k_nmf_gather<true, false>), dim3(grid), dim3(kBlock), 0, s, *p, src, R, d, dm, pointwise,
                                ctx->X[0], ctx->G, thresh, scale, seed, stats);
    } else {
        if (H) hipLaunchKernelGGL((k_nmf_gather<false, true>), dim3(grid), dim3(kBlock), 0, s, *p, src, R, d, dm, 0, ctx->X[0],
                                  ctx->G, 0u, 1.f, (uint64_t)0, (double *)nullptr);
        else hipLaunchKernelGGL((k_nmf_gather<false, false>), dim3(grid), dim3(kBlock), 0, s, *p, src, R, d, dm, 0, ctx->X[0],
                                ctx->G, 0u, 1.f, (uint64_t)0, (double *)nullptr);
    }
    DAISY_LAUNCH_CHECK();
    if (ctx->model != DAISY_NEUMF_GMF) {
        for (int l = path.fact ? 2 : 1; l <= L; ++l) {        // (fact: x1 came out of the gather)
            GemmOp op{};
            op.A = ctx->X[l - 1]; op.sam = ctx->width[l - 1]; op.sak = 1;
            op.B = p->W[l - 1]; op.sbn = ctx->width[l - 1]; op.sbk = 1;
            op.C = ctx->X[l]; op.ldc = ctx->width[l];
            op.M = R; op.N = ctx->width[l]; op.K = ctx->width[l - 1];
            op.bias = p->b[l - 1];
            op.k_chunk = op.K;
            op.bf16 = ctx->bf16 ? 1 : 0;
            if (l < L && thresh) {       // the Dropout in front of Linear l+1 acts on this output
                op.drop_thresh = thresh; op.drop_scale = scale; op.drop_seed = seed; op.drop_stream = (uint32_t)(l + 1);
            }
            if (H) {
                op.A16 = reinterpret_cast<const uint16_t *>(ctx->X[l - 1]);
                op.B16 = ctx->W16[l - 1];
                op.C16 = reinterpret_cast<uint16_t *>(ctx->X[l]);
                if (!gemm_h_ok(op)) { set_error("neumf: layer %d does not tile for the bf16-storage GEMM", l); return DAISY_ERR_STATE; }
                launch_gemm_h<EPI_BIAS_RELU>(op, s);
            } else {
                launch_gemm<EPI_BIAS_RELU>(op, s);
            }
            DAISY_LAUNCH_CHECK();
        }
    }
    const int dg = (ctx->model == DAISY_NEUMF_MLP) ? 0 : d;
    const int nl = (ctx->model == DAISY_NEUMF_GMF) ? 0 : ctx->width[L];
    if (H) hipLaunchKernelGGL((k_nmf_predict<true>), dim3(grid), dim3(kBlock), 0, s, ctx->G, dg, ctx->X[L], nl, p->Wp, p->bp, R,
                              ctx->pred);
    else hipLaunchKernelGGL((k_nmf_predict<false>), dim3(grid), dim3(kBlock), 0, s, ctx->G, dg, ctx->X[L], nl, p->Wp, p->bp, R,
                            ctx->pred);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

// ---------------------------------------------------------------------------------------------
// the backward pass of a training step, piece by piece (daisy_neumf_step_grads puts them in order)
// ---------------------------------------------------------------------------------------------
struct NeumfStep {                           // a step's arguments, as the pieces take them
    const int32_t *u, *i, *j;
    int64_t B, R;
    int pointwise, loss_type;
    float gamma, reg_1, reg_2;
    uint32_t thresh;                         // dropout: keep threshold (0: off), scale, seed
    float scale;
    uint64_t seed;
    double *stats;
    hipStream_t s;
};

static MidArgs neumf_mid_args(const daisy_neumf_ctx *ctx, const daisy_neumf_params &p, const NeumfStep &st, float *dx0) {
    MidArgs ma{};
    ma.uG = p.uG; ma.iG = p.iG; ma.uM = p.uM; ma.iM = p.iM; ma.u = st.u; ma.i = st.i; ma.dm = ctx->dm;
    ma.DX0 = dx0; ma.pred = ctx->pred; ma.dpred = ctx->dpred;
    for (int l = 0; l < ctx->L; ++l) { ma.W[l] = p.W[l]; ma.b[l] = p.b[l]; }
    ma.Wp = p.Wp; ma.bp = p.bp;
    for (int l = 0; l <= ctx->L; ++l) ma.width[l] = ctx->width[l];
    ma.L = ctx->L; ma.d = ctx->d;
    ma.j = st.j; ma.B = (int)st.B; ma.R = (int)st.R; ma.pointwise = st.pointwise; ma.loss_type = st.loss_type; ma.gamma = st.gamma;
    ma.thresh = st.thresh; ma.scale = st.scale; ma.seed = st.seed;
    ma.ws = ctx->det_ws;
    return ma;
}

// x1 gathered from the table products, layers 2..3, predict, criterion, dZ3 .. dZ1, gW3, gW2, gb3, gb2, gWp, gbp and the
// step's statistics: one persistent kernel + the fixed-order sum of its workgroups' slabs
static TowerArgs neumf_tower_args(const daisy_neumf_ctx *ctx, const daisy_neumf_params &p, const NeumfStep &st, const Fact &fact,
                                  float *dz1) {
    TowerArgs ta{};
    ta.tu = fact.tu; ta.ti = fact.ti; ta.nu = fact.nu; ta.ni = fact.ni;
    ta.b1 = p.b[0];
    ta.W2 = p.W[1]; ta.W3 = p.W[2];
    ta.b2 = p.b[1]; ta.b3 = p.b[2]; ta.Wp = p.Wp; ta.bp = p.bp;
    ta.uG = p.uG; ta.iG = p.iG;
    ta.u = st.u; ta.i = st.i; ta.j = st.j; ta.B = st.B;
    ta.pointwise = st.pointwise; ta.loss_type = st.loss_type; ta.gamma = st.gamma;
    ta.dZ1 = reinterpret_cast<uint16_t *>(dz1); ta.dpred = ctx->dpred; ta.ws = ctx->det_ws;
    return ta;
}

// the layered path's criterion and predict-layer backward: dpred, the loss and the norms, gbp, gWp, and dZ_L into dz
static int neumf_head_bwd(daisy_neumf_ctx *ctx, const daisy_neumf_params &p, const daisy_neumf_params &g, const NeumfPath &path,
                          const NeumfStep &st, float *dz) {
    const int L = ctx->L;
    const int64_t R = st.R;
    hipStream_t s = st.s;
    float *ws = ctx->det_ws;
    const int loss_grid = grid_for(st.B, kBlock * 2);
    hipLaunchKernelGGL(k_nmf_loss, dim3(loss_grid), dim3(kBlock), 0, s, ctx->pred, st.j, st.B, st.loss_type, st.gamma, st.pointwise,
                       ctx->dpred, st.stats, ws);
    reduce_slices(ws, loss_grid, 1, g.bp, s);
    hipLaunchKernelGGL(k_nmf_finalize, dim3(1), dim3(64), 0, s, st.stats, st.reg_1, st.reg_2, st.pointwise);
    DAISY_LAUNCH_CHECK();
    const int dg = (ctx->model == DAISY_NEUMF_MLP) ? 0 : ctx->d;
    const int nl = (ctx->model == DAISY_NEUMF_GMF) ? 0 : ctx->width[L];
    const bool vec_pred = dg == nl && dg > 0 && dg <= 64 && dg % 4 == 0;          // NeuMF proper (not the GMF / MLP ablations)
    const int pb_grid = vec_pred ? grid_for(R, kBlock / 16 * 8, 512) : grid_for(R, kBlock / 16 * 16, 1024);
    if (vec_pred && path.H) hipLaunchKernelGGL((k_nmf_pred_bwd_v<true>), dim3(pb_grid), dim3(kBlock), 0, s, ctx->dpred, ctx->G, dg,
                                               ctx->X[L], p.Wp, R, dz, ws);
    else if (vec_pred) hipLaunchKernelGGL((k_nmf_pred_bwd_v<false>), dim3(pb_grid), dim3(kBlock), 0, s, ctx->dpred, ctx->G, dg,
                                          ctx->X[L], p.Wp, R, dz, ws);
    else if (path.H) hipLaunchKernelGGL((k_nmf_pred_bwd<true>), dim3(pb_grid), dim3(kBlock), 0, s, ctx->dpred,
                                        ctx->G, dg, ctx->X[L], nl, p.Wp, R, dz, ws);
    else hipLaunchKernelGGL((k_nmf_pred_bwd<false>), dim3(pb_grid), dim3(kBlock), 0, s, ctx->dpred,
                            ctx->G, dg, ctx->X[L], nl, p.Wp, R, dz, ws);
    reduce_slices(ws, pb_grid, dg + nl, g.Wp, s);       // gWp += the workgroups' column sums, in workgroup order
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

// layer l backward: gW_l += dZ_l^T x_{l-1}, gb_l += the column sums of dZ_l (dz), dZ_{l-1} = (dZ_l W_l) gated into dz_next
static int neumf_layer_bwd(daisy_neumf_ctx *ctx, const daisy_neumf_params &p, const daisy_neumf_params &g, const NeumfPath &path,
                           const NeumfStep &st, int l, float *dz, float *dz_next) {
    const int n_out = ctx->width[l], n_in = ctx->width[l - 1];
    const int64_t R = st.R;
    hipStream_t s = st.s;
    float *ws = ctx->det_ws;
    GemmOp w{};                                   // gW_l[n_out, n_in] += dZ^T x_{l-1}
    if (n_out % kGemmBM == 0) {
        w.A = dz; w.sam = 1; w.sak = n_out;
        w.B = ctx->X[l - 1]; w.sbn = 1; w.sbk = n_in;
        w.ldc = n_in;
        w.M = n_out; w.N = n_in;
    } else {                                      // narrow layer: tile the wider side over M, store transposed
        w.A = ctx->X[l - 1]; w.sam = 1; w.sak = n_in;
        w.B = dz; w.sbn = 1; w.sbk = n_out;
        w.ldc = 1; w.scn = n_in;
        w.M = n_in; w.N = n_out;
    }
    w.K = R;
    w.k_chunk = wgrad_chunk();
    {
        // few rows (the reference's own batch: 256 samples = 512 rows) and a small layer: ONE workgroup would walk all
        // rows of the step with guarded loads - 50 us per weight gradient at factors 24, a third of that step.  Slices
        // of at least 64 rows, as many as give the chip ~256 workgroups and as the reduction workspace holds.
        const int64_t tiles = ((w.M + kGemmBM - 1) / kGemmBM) * ((w.N + ((w.N > 64) ? 128 : 64) - 1) / ((w.N > 64) ? 128 : 64));
        int64_t kc = (R * tiles / 256 + 63) / 64 * 64;
        if (kc < 64) kc = 64;
        const int64_t cap = (int64_t)(ctx->det_ws_floats / (size_t)((int64_t)n_out * n_in));
        if (cap > 0 && (R + kc - 1) / kc > cap) kc = ((R + cap - 1) / cap + 63) / 64 * 64;
        if (kc < w.k_chunk) w.k_chunk = kc;
    }
    w.bf16 = ctx->bf16 ? 1 : 0;
    // split-K slices land side by side in the workspace and are added in slice order (no fp32 atomics)
    const int64_t wlen = (int64_t)n_out * n_in;
    const int wsplits = (int)((w.k_chunk < R) ? (R + w.k_chunk - 1) / w.k_chunk : 1);
    w.C = ws;
    w.slice_stride = wlen;
    const int cr = colsum_rows(R);
    const dim3 cs_grid((unsigned)((n_out + 63) / 64), (unsigned)((R + cr - 1) / cr));
    GemmOp x{};                                   // dZ_{l-1}[R, n_in] = (dZ W_l) gated
    x.A = dz; x.sam = n_out; x.sak = 1;
    x.B = p.W[l - 1]; x.sbn = 1; x.sbk = n_in;
    x.C = dz_next; x.ldc = n_in;
    x.M = R; x.N = n_in; x.K = n_out;
    x.k_chunk = x.K;
    x.bf16 = ctx->bf16 ? 1 : 0;
    if (l > 1) {                                  // ReLU (and dropout) gate of x_{l-1}
        x.gate = ctx->X[l - 1]; x.ldg = n_in; x.gate_scale = st.scale;
    } else if (st.thresh) {                       // dropout mask of the concat input
        x.drop_thresh = st.thresh; x.drop_scale = st.scale; x.drop_seed = st.seed; x.drop_stream = 1u;
    }
    if (path.H) {
        w.A16 = reinterpret_cast<const uint16_t *>(w.A);
        w.B16 = reinterpret_cast<const uint16_t *>(w.B);
        if (!gemm_h_ok(w)) { set_error("neumf: weight gradient of layer %d does not tile for the bf16-storage GEMM", l); return DAISY_ERR_STATE; }
        launch_gemm_h<EPI_ATOMIC>(w, s);
        reduce_slices(ws, wsplits, wlen, g.W[l - 1], s);
        if (n_out % 8 == 0 && kBlock % (n_out / 8) == 0) {
            const int tiles = (int)((R + kColsumRowsH - 1) / kColsumRowsH);
            hipLaunchKernelGGL(k_colsum_h, dim3((unsigned)tiles), dim3(kBlock), 0, s, reinterpret_cast<const uint16_t *>(dz), R, n_out, ws);
            reduce_slices(ws, tiles, n_out, g.b[l - 1], s);
        } else {
            hipLaunchKernelGGL((k_colsum<true>), cs_grid, dim3(kBlock), 0, s, dz, R, n_out, (int64_t)n_out, ws, cr);
            reduce_slices(ws, (int)cs_grid.y, n_out, g.b[l - 1], s);
        }
        x.A16 = reinterpret_cast<const uint16_t *>(dz);
        x.B16 = ctx->W16T[l - 1]; x.sbn = n_out; x.sbk = 1;        // W^T [n_in][n_out]: both operands along k
        x.C16 = reinterpret_cast<uint16_t *>(dz_next);        // bf16 like every other stored gradient of this level
        x.G16 = (l > 1) ? reinterpret_cast<const uint16_t *>(ctx->X[l - 1]) : nullptr;
        if (!gemm_h_ok(x)) { set_error("neumf: input gradient of layer %d does not tile for the bf16-storage GEMM", l); return DAISY_ERR_STATE; }
        launch_gemm_h<EPI_GATE>(x, s);
    } else {
        launch_gemm<EPI_ATOMIC>(w, s);
        reduce_slices(ws, wsplits, wlen, g.W[l - 1], s);
        hipLaunchKernelGGL((k_colsum<false>), cs_grid, dim3(kBlock), 0, s, dz, R, n_out, (int64_t)n_out, ws, cr);
        reduce_slices(ws, (int)cs_grid.y, n_out, g.b[l - 1], s);
        launch_gemm<EPI_GATE>(x, s);
    }
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

// The first layer through the tables, backward (path.fact), after the scatter: it left S_u / S_i - the segment sums of dZ_1 by
// user / by item, fp32 [rows, n1] - in its two MLP row-sum tables.  gb_1 = the column sums of S_u,  g.table += S W1[:, half]  and
// gW_1[:, half] += S^T table: two GEMMs over the TABLE's rows where the plain path runs one over the step's R rows and a
// [R, 2 dm] input gradient.  Both sum tables are all-zero again afterwards.
static int neumf_first_layer_bwd(daisy_neumf_ctx *ctx, const daisy_neumf_params &p, const daisy_neumf_params &g, hipStream_t s) {
    // every product runs for both sides in ONE launch (k_gemm_pair: each side alone is a latency-bound ~100 workgroups)
    const int dm = ctx->dm, n1 = dm, w0 = 2 * dm;
    const NeumfScatter &sc = ctx->scatter;
    {   // gb_1 = sum over the step's rows of dZ_1 = sum over the USERS of their segment sums: a column sum over U table rows
        // (6 MB at ml-1m) instead of one over the R rows of dZ_1 (268 MB: 47 us)
        const int cr = colsum_rows(ctx->U);
        const dim3 cs((unsigned)((n1 + 63) / 64), (unsigned)((ctx->U + cr - 1) / cr));
        hipLaunchKernelGGL((k_colsum<false>), cs, dim3(kBlock), 0, s, sc.sum, ctx->U, n1, (int64_t)n1, ctx->det_ws, cr);
        reduce_slices(ctx->det_ws, (int)cs.y, n1, g.b[0], s);
    }
    GemmOp a[2], b[2];
    // slices of 128 table rows while the workspace holds both sides' slices; tables with more rows than that (the
    // workspace is sized by the step's rows) take proportionally longer slices - never an error mid-step
    const int64_t cap = (int64_t)(ctx->det_ws_floats / ((size_t)n1 * (size_t)dm));      // >= 2
    int64_t kc = 128;
    while ((ctx->U + kc - 1) / kc + (ctx->I + kc - 1) / kc > cap) kc += 128;
    int bsplits[2];
    for (int side = 0; side < 2; ++side) {
        const int64_t rows = side ? ctx->I : ctx->U;
        float *S = side ? sc.sum2 : sc.sum;
        a[side] = GemmOp{};                // g.table[rows, dm] += S[rows, n1] W1[:, half]      (k = n1)
        a[side].A = S; a[side].sam = n1; a[side].sak = 1;
        a[side].B = p.W[0] + (side ? dm : 0); a[side].sbn = 1; a[side].sbk = w0;
        a[side].C = side ? g.iM : g.uM; a[side].ldc = dm;
        a[side].M = rows; a[side].N = dm; a[side].K = n1; a[side].k_chunk = n1;
        b[side] = GemmOp{};                // gW_1[n1, half] += S^T[n1, rows] table[rows, dm]    (k = the table's rows, in slices)
        b[side].A = S; b[side].sam = 1; b[side].sak = n1;
        b[side].B = side ? p.iM : p.uM; b[side].sbn = 1; b[side].sbk = dm;
        b[side].M = n1; b[side].N = dm; b[side].K = rows; b[side].k_chunk = kc;
        bsplits[side] = (int)((rows + kc - 1) / kc);
        b[side].C = ctx->det_ws + (side ? (size_t)bsplits[0] * n1 * dm : 0); b[side].ldc = dm; b[side].slice_stride = (int64_t)n1 * dm;
    }
    launch_gemm_pair<EPI_ATOMIC>(a[0], a[1], s);       // (one workgroup per output tile, k in one piece: a single add per element)
    launch_gemm_pair<EPI_ATOMIC>(b[0], b[1], s);
    hipLaunchKernelGGL(k_reduce_slices_2d, dim3(grid_for((int64_t)n1 * dm, kBlock, 2048), 2), dim3(kBlock), 0, s, b[0].C, bsplits[0], n1,
                       dm, g.W[0], (int64_t)w0, (const float *)b[1].C, bsplits[1], g.W[0] + dm);
    // (both sum tables back to all-zero: they are contiguous)
    DAISY_HIP(hipMemsetAsync(sc.sum, 0, (size_t)((char *)sc.sumg - (char *)sc.sum), s));
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

extern "C" {

int daisy_neumf_ctx_create(daisy_neumf_ctx **out, int64_t max_rows, int32_t factors, int32_t num_layers,
                           int32_t model, int64_t user_num, int64_t item_num) {
    DAISY_CHECK_ARG(out != nullptr, "neumf_ctx_create: out is NULL");
    *out = nullptr;
    DAISY_CHECK_ARG(max_rows > 0 && user_num > 0 && item_num > 0, "neumf_ctx_create: bad sizes");
    DAISY_CHECK_ARG(factors > 0 && factors % 4 == 0 && factors <= 256,
                    "neumf_ctx_create: factors=%d must be a multiple of 4 in 4..256", factors);
    DAISY_CHECK_ARG(num_layers >= 1 && num_layers <= DAISY_NEUMF_MAX_LAYERS, "neumf_ctx_create: num_layers=%d",
                    num_layers);
    DAISY_CHECK_ARG(model >= DAISY_NEUMF_FULL && model <= DAISY_NEUMF_MLP, "neumf_ctx_create: model=%d", model);
    daisy_neumf_ctx *c = new daisy_neumf_ctx();
    c->max_rows = max_rows; c->U = user_num; c->I = item_num;
    c->d = factors; c->L = num_layers; c->model = model;
    c->bf16 = 0;
    c->det_ws = nullptr; c->det_ws_floats = 0;
    c->dm = factors << (num_layers - 1);
    c->width[0] = 2 * c->dm;
    for (int l = 1; l <= num_layers; ++l) c->width[l] = c->width[l - 1] / 2;
    c->mid_fits = neumf_mid_fits(c->L, c->width, c->d);
    c->scatter.max_rows = max_rows; c->scatter.U = user_num; c->scatter.I = item_num;
    c->scatter.d = c->d; c->scatter.dm = c->dm; c->scatter.model = model;
    DeviceArena &a = c->arena;
    for (int l = 0; l <= num_layers; ++l) a.add(&c->X[l], (size_t)max_rows * c->width[l] * 4);
    a.add(&c->G, (size_t)max_rows * factors * 4);
    a.add(&c->pred, (size_t)max_rows * 4);
    a.add(&c->dpred, (size_t)max_rows * 4);
    a.add(&c->DZ[0], (size_t)max_rows * c->width[0] * 4);
    a.add(&c->DZ[1], (size_t)max_rows * c->width[0] * 4);
    for (int l = 1; l <= num_layers; ++l) a.add(&c->W16[l - 1], (size_t)c->width[l] * c->width[l - 1] * 2 * 2);
    if (int rc = a.alloc("neumf_ctx_create")) {
        delete c;
        return rc;
    }
    for (int l = 1; l <= num_layers; ++l) c->W16T[l - 1] = c->W16[l - 1] + (size_t)c->width[l] * c->width[l - 1];
    *out = c;
    return DAISY_OK;
}

int daisy_neumf_ctx_destroy(daisy_neumf_ctx *ctx) {
    if (!ctx) return DAISY_OK;
    ctx->arena.release();
    neumf_scatter_release(ctx->scatter);
    if (ctx->det_ws) (void)hipFree(ctx->det_ws);
    if (ctx->fact_t) (void)hipFree(ctx->fact_t);
    delete ctx;
    return DAISY_OK;
}

size_t daisy_neumf_ctx_bytes(const daisy_neumf_ctx *ctx) { return ctx ? ctx->arena.bytes() : 0; }

int daisy_neumf_ctx_set_precision(daisy_neumf_ctx *ctx, int32_t bf16_gemm) {
    DAISY_CHECK_ARG(ctx != nullptr, "neumf_ctx_set_precision: NULL context");
    DAISY_CHECK_ARG(bf16_gemm >= 0 && bf16_gemm <= 2, "neumf_ctx_set_precision: level %d not in 0..2", bf16_gemm);
    ctx->bf16 = bf16_gemm;
    return DAISY_OK;
}


int daisy_neumf_scores(daisy_neumf_ctx *ctx, const daisy_neumf_params *params, const int64_t *users,
                       const int64_t *items, int64_t n, int64_t C, float *out, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && params && users && out && n > 0 && C >= 0, "neumf_scores: bad argument");
    DAISY_CHECK_ARG(items || C == 0, "neumf_scores: items is NULL but C != 0");
    hipStream_t s = as_stream(stream);
    for (int64_t base = 0; base < n; base += ctx->max_rows) {
        const int64_t R = (n - base < ctx->max_rows) ? (n - base) : ctx->max_rows;
        PairSrc src{};
        src.users = users; src.items = items; src.C = C; src.base = base;
        const NeumfPath path = neumf_path(ctx, *params, R, false, 0u);
        int rc = neumf_forward_rows(ctx, params, path, src, R, false, 0, 0u, 1.f, 0, nullptr, nullptr, s);
        if (rc) return rc;
        DAISY_HIP(hipMemcpyAsync(out + base, ctx->pred, (size_t)R * 4, hipMemcpyDeviceToDevice, s));
    }
    return DAISY_OK;
}

int daisy_neumf_scores_users(daisy_neumf_ctx *ctx, const daisy_neumf_params *params, const int64_t *users, int64_t m,
                             float *out, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && params && users && out && m > 0, "neumf_scores_users: bad argument");
    DAISY_CHECK_ARG(m <= INT64_MAX / ctx->I, "neumf_scores_users: m=%lld users x %lld items overflow", (long long)m,
                    (long long)ctx->I);
    hipStream_t s = as_stream(stream);
    const int64_t n = m * ctx->I;
    for (int64_t base = 0; base < n; base += ctx->max_rows) {
        const int64_t R = (n - base < ctx->max_rows) ? (n - base) : ctx->max_rows;
        PairSrc src{};
        src.users = users; src.all_items = ctx->I; src.base = base;
        const NeumfPath path = neumf_path(ctx, *params, R, false, 0u);
        int rc = neumf_forward_rows(ctx, params, path, src, R, false, 0, 0u, 1.f, 0, nullptr, nullptr, s);
        if (rc) return rc;
        DAISY_HIP(hipMemcpyAsync(out + base, ctx->pred, (size_t)R * 4, hipMemcpyDeviceToDevice, s));
    }
    return DAISY_OK;
}

int daisy_neumf_step_grads(daisy_neumf_ctx *ctx, const daisy_neumf_params *params,
                           const daisy_neumf_params *grads, const int32_t *u, const int32_t *i,
                           const int32_t *j, int64_t B, int32_t loss_type, float gamma, float reg_1,
                           float reg_2, float dropout_p, uint64_t seed, double *stats,
                           daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && params && grads && u && i && j && stats && B > 0, "neumf_step_grads: bad argument");
    DAISY_CHECK_ARG(loss_type >= DAISY_LOSS_BPR && loss_type <= DAISY_LOSS_SL, "Invalid loss type: %d", loss_type);
    DAISY_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "neumf_step_grads: dropout_p=%g not in [0,1)", dropout_p);
    const int pointwise = loss_type >= DAISY_LOSS_CL;
    const int64_t R = pointwise ? B : 2 * B;
    DAISY_CHECK_ARG(R <= ctx->max_rows, "neumf_step_grads: %lld rows exceed the context's %lld",
                    (long long)R, (long long)ctx->max_rows);
    hipStream_t s = as_stream(stream);
    const daisy_neumf_params &p = *params, &g = *grads;
    const uint32_t thresh = (ctx->model == DAISY_NEUMF_GMF) ? 0u : keep_threshold(dropout_p);
    const NeumfStep st{u, i, j, B, R, pointwise, (int)loss_type, gamma, reg_1, reg_2, thresh, thresh ? 1.f / (1.f - dropout_p) : 1.f,
                       seed, stats, s};
    const NeumfPath path = neumf_path(ctx, p, R, true, thresh);
    // (slots 0..16: DAISY_NST_LOSS_SUM runs over steps; the small-step path writes every slot itself - k_nmf_mid_reduce -
    // and so does the fused tower: k_nmf_tower_reduce)
    if (!path.mid && !path.tower) DAISY_HIP(hipMemsetAsync(stats, 0, DAISY_NST_LOSS_SUM * sizeof(double), s));
    PairSrc src{};
    src.u = u; src.i = i; src.j = pointwise ? i : j; src.B = B;
    Fact fact{};
    int rc = neumf_forward_rows(ctx, params, path, src, R, true, pointwise, thresh, st.scale, seed, stats, &fact, s);
    if (rc) return rc;
    if ((rc = neumf_need_det_ws(ctx))) return rc;
    float *dz = ctx->DZ[0], *dz_next = ctx->DZ[1];
    // the head: criterion and predict layer - the two fused kernels run it together with the layers they cover
    if (path.mid) rc = neumf_mid_step(neumf_mid_args(ctx, p, st, dz), g.W, g.b, g.Wp, g.bp, stats, reg_1, reg_2, s);
    else if (path.tower) rc = neumf_tower_step(neumf_tower_args(ctx, p, st, fact, dz), ctx->d, R, g.W[1], g.W[2], g.b[1], g.b[2], g.Wp, g.bp,
                                               stats, reg_1, reg_2, s);
    else rc = neumf_head_bwd(ctx, p, g, path, st, dz);
    if (rc) return rc;
    // the layers: none under mid (dz already holds dX0) and under the tower (dz already holds dZ_1); the first one not under
    // fact - gb_1, gW_1 and the MLP tables' gradients then come from the segmented sums of dZ_1 (neumf_first_layer_bwd): no
    // [R, 2 dm] input gradient, no weight-gradient GEMM over the R rows
    if (ctx->model != DAISY_NEUMF_GMF && !path.mid)
        for (int l = path.tower ? 1 : ctx->L; l >= (path.fact ? 2 : 1); --l) {
            if ((rc = neumf_layer_bwd(ctx, p, g, path, st, l, dz, dz_next))) return rc;
            float *t = dz; dz = dz_next; dz_next = t;
        }
    if ((rc = neumf_scatter(ctx->scatter, path, p, g, src, R, pointwise, ctx->dpred, dz, stats, reg_1, reg_2, s))) return rc;
    return path.fact ? neumf_first_layer_bwd(ctx, p, g, s) : DAISY_OK;
}

int daisy_neumf_fit_epoch(daisy_neumf_ctx *ctx, const daisy_neumf_params *params, const daisy_neumf_params *grads,
                          const int32_t *u, const int32_t *i, const int32_t *j, int64_t n, int64_t batch, int32_t loss_type,
                          float gamma, float reg_1, float reg_2, float dropout_p, uint64_t seed_hi, int64_t step0,
                          int32_t optimizer, float lr, float *W, float *g, float *state0, float *state1, int64_t n_flat,
                          double *stats, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && params && grads && u && i && j && stats && W && g && n > 0 && batch > 0 && n_flat > 0 && step0 >= 0,
                    "neumf_fit_epoch: bad argument");
    if (int rc = dense_opt_check("neumf_fit_epoch", optimizer, state0, state1)) return rc;
    // the reference's loop (AbstractRecommender.py:119-128) over the epoch's batches, issued from here: at 256 samples per step
    // a step is ~40 us of kernels, less than the Python of one iteration around two library calls
    int64_t step = step0;
    for (int64_t s0 = 0; s0 < n; s0 += batch) {
        const int64_t B = (n - s0 < batch) ? n - s0 : batch;
        ++step;
        int rc = daisy_neumf_step_grads(ctx, params, grads, u + s0, i + s0, j + s0, B, loss_type, gamma, reg_1, reg_2, dropout_p,
                                        seed_hi | (uint64_t)step, stats, stream);
        if (rc) return rc;
        // (Adam's step count here is the dropout step counter itself: this entry point has no separate opt_step0)
        if ((rc = dense_opt_step(optimizer, W, g, state0, state1, n_flat, lr, step, stream))) return rc;
    }
    return DAISY_OK;
}

}  // extern "C"
