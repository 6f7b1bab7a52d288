// NGCF (daisy/model/NGCFRecommender.py:38-172) on gfx950: the dense bi-interaction layer over all N = U + I nodes.
//   forward  k_ngcf_layer_fwd:  Z = [E + X | X * E] [W1 | W2]^T + b1 + b2 (f32 MFMA, K = 2 d_in), then in registers
//                               LeakyReLU(0.2), message dropout, the row L2 norm and the scale.  Per row it reads
//                               2 d_in floats and writes d_out (+ the norm).
//   backward k_ngcf_layer_bwd:  dZ from dY, Y, norm (normalize / dropout / LeakyReLU backward, staged in LDS), then
//                               [dS | dT] = dZ [W1 | W2] (f32 MFMA) and dE = gprev + dS + dT * X, dX = dS + dT * E.
//            k_ngcf_wgrad:      per row chunk, the partial [dW1 | dW2] = dZ^T [S | T] and db = sum dZ (f32 MFMA);
//            k_ngcf_wgrad_sum:  the chunks summed in chunk order - no float atomics, so the weight gradients repeat
//                               bit for bit.
// Everything is fp32 like the reference.  The sparse products (X = A_hat E and its transpose) are
// daisy_lgcn_spmm_ex in lightgcn.hip.
#include "common.h"
#include "mfma.h"

namespace daisy {

constexpr int kNgRows = 128;    // forward: rows per tile (4 waves x 32)
constexpr int kNgKC = 16;       // forward: K chunk staged in LDS
constexpr int kNgBRows = 64;    // backward: rows per tile (2 row blocks x 2 column halves)
constexpr int kNgWRows = 16;    // weight gradient: rows per staged slice
constexpr int kNgMaxNB = DAISY_NGCF_MAX_WIDTH / 32;

__device__ __forceinline__ floatx16 mfma32(float a, float b, floatx16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
// row of register q of a 32x32 MFMA result in lane half h (column = lane & 31)
__device__ __forceinline__ int mrow(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

struct NgFwd {
    const float *E;
    int64_t lde;
    const float *X, *W1, *b1, *W2, *b2;
    float *Y;
    int64_t ldy;
    float *norm;
    int64_t n;
    int din, dout;
    uint32_t thresh, stream;
    float scale;
    uint64_t seed;
};

// NB = ceil(d_out / 32): every wave owns 32 rows of the tile and all d_out columns (NB accumulators)
template <int NB>
__global__ __launch_bounds__(kBlock) void k_ngcf_layer_fwd(NgFwd a) {
    __shared__ float sA[2][kNgRows][kNgKC + 1];        // S and T chunks [row][k]
    __shared__ float sW[2][kNgKC][NB * 32];            // W1^T and W2^T chunks [k][out]
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave, lc = lane & 31, lh = lane >> 5;
    const int kpad = (a.din + kNgKC - 1) / kNgKC * kNgKC;
    const int64_t ntiles = (a.n + kNgRows - 1) / kNgRows;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * kNgRows;
        floatx16 acc[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[nb][q] = 0.f;
        for (int kc = 0; kc < kpad; kc += kNgKC) {
            __syncthreads();
            for (int idx = threadIdx.x; idx < kNgRows * kNgKC; idx += kBlock) {
                const int r = idx / kNgKC, c = idx % kNgKC, k = kc + c;
                const int64_t gr = row0 + r;
                float e = 0.f, x = 0.f;
                if (gr < a.n && k < a.din) {
                    e = a.E[gr * a.lde + k];
                    x = a.X[gr * a.din + k];
                }
                sA[0][r][c] = e + x;
                sA[1][r][c] = x * e;
            }
            for (int idx = threadIdx.x; idx < NB * 32 * kNgKC; idx += kBlock) {
                const int o = idx / kNgKC, c = idx % kNgKC, k = kc + c;
                float w1 = 0.f, w2 = 0.f;
                if (o < a.dout && k < a.din) {
                    w1 = a.W1[(int64_t)o * a.din + k];
                    w2 = a.W2[(int64_t)o * a.din + k];
                }
                sW[0][c][o] = w1;
                sW[1][c][o] = w2;
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < kNgKC; kk += 2) {
                const float aS = sA[0][wave * 32 + lc][kk + lh], aT = sA[1][wave * 32 + lc][kk + lh];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    acc[nb] = mfma32(aS, sW[0][kk + lh][nb * 32 + lc], acc[nb]);
                    acc[nb] = mfma32(aT, sW[1][kk + lh][nb * 32 + lc], acc[nb]);
                }
            }
        }
        // epilogue in registers: bias, LeakyReLU, dropout, row sum of squares over the 32 lanes of each half
        float ss[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) ss[q] = 0.f;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int col = nb * 32 + lc;
            const bool valid = col < a.dout;
            const float bb = valid ? a.b1[col] + a.b2[col] : 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int64_t gr = row0 + wave * 32 + mrow(q, lh);
                const float z = acc[nb][q] + bb;
                float h = z > 0.f ? z : 0.2f * z;
                if (a.thresh)
                    h = drop_keep(a.seed, a.stream, (uint64_t)gr * (uint64_t)a.dout + (uint64_t)col, a.thresh) ? h * a.scale
                                                                                                               : 0.f;
                h = valid ? h : 0.f;
                acc[nb][q] = h;
                ss[q] = fmaf(h, h, ss[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q)
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) ss[q] += __shfl_xor(ss[q], off);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int64_t gr = row0 + wave * 32 + mrow(q, lh);
            if (gr >= a.n) continue;
            const float nrm = sqrtf(ss[q]);
            const float den = fmaxf(nrm, 1e-12f);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int col = nb * 32 + lc;
                if (col < a.dout) a.Y[gr * a.ldy + col] = acc[nb][q] / den;
            }
            if (lc == 0) a.norm[gr] = nrm;
        }
    }
}

struct NgBwd {
    const float *dY;
    int64_t ldd;
    const float *Y;
    int64_t ldy;
    const float *norm, *E;
    int64_t lde;
    const float *X, *W1, *W2, *gprev;
    int64_t ldg;
    float *dE, *dX, *dZ;
    int64_t n;
    int din, dout;
    uint32_t thresh, stream;
    float scale;
    uint64_t seed;
};

// TPW = input column blocks per wave: wave w owns row block (w & 1) of the 64-row tile and the d_in column blocks
// nb = (w >> 1) + 2 t, t < TPW, for both dS and dT (the epilogue needs both of a column in one lane)
template <int TPW>
__global__ __launch_bounds__(kBlock) void k_ngcf_layer_bwd(NgBwd a) {
    __shared__ float sDZ[kNgBRows][DAISY_NGCF_MAX_WIDTH + 1];
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave, lc = lane & 31, lh = lane >> 5;
    const int nbo = (a.dout + 31) / 32, nbi = (a.din + 31) / 32;
    const int64_t ntiles = (a.n + kNgBRows - 1) / kNgBRows;
    const int l32 = threadIdx.x % 32, rsub = threadIdx.x / 32;      // phase 1: 8 rows per pass, 32 lanes per row
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * kNgBRows;
        __syncthreads();
        // phase 1: dZ of the tile into LDS (and to global for the weight gradient)
        for (int p = 0; p < kNgBRows / 8; ++p) {
            const int r = p * 8 + rsub;
            const int64_t gr = row0 + r;
            const bool rv = gr < a.n;
            float yv[kNgMaxNB], dv[kNgMaxNB], dot = 0.f;
#pragma unroll
            for (int j = 0; j < kNgMaxNB; ++j) {
                const int c = l32 + 32 * j;
                const bool ok = rv && c < a.dout;
                yv[j] = ok ? a.Y[gr * a.ldy + c] : 0.f;
                dv[j] = ok ? a.dY[gr * a.ldd + c] : 0.f;
                dot = fmaf(yv[j], dv[j], dot);
            }
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) dot += __shfl_xor(dot, off);
            const float nrm = rv ? a.norm[gr] : 1.f;
            const bool big = nrm >= 1e-12f;
#pragma unroll
            for (int j = 0; j < kNgMaxNB; ++j) {
                const int c = l32 + 32 * j;
                const bool ok = rv && c < a.dout;
                float g = big ? (dv[j] - yv[j] * dot) / nrm : dv[j] / 1e-12f;      // F.normalize backward
                if (a.thresh)
                    g = drop_keep(a.seed, a.stream, (uint64_t)gr * (uint64_t)a.dout + (uint64_t)c, a.thresh) ? g * a.scale
                                                                                                             : 0.f;
                float dz = yv[j] > 0.f ? g : 0.2f * g;          // sign(Z) = sign(Y) wherever the element was kept
                dz = ok ? dz : 0.f;
                sDZ[r][c] = dz;
                if (ok) a.dZ[gr * a.dout + c] = dz;
            }
        }
        __syncthreads();
        // phase 2: [dS | dT] = dZ [W1 | W2] on MFMA, W streamed from L2
        const int rb = wave & 1, cs = wave >> 1;
        floatx16 aS[TPW], aT[TPW];
#pragma unroll
        for (int t = 0; t < TPW; ++t)
#pragma unroll
            for (int q = 0; q < 16; ++q) { aS[t][q] = 0.f; aT[t][q] = 0.f; }
        for (int o0 = 0; o0 < nbo * 32; o0 += 2) {
            const int ko = o0 + lh;
            const float av = sDZ[rb * 32 + lc][ko];
            const bool kv = ko < a.dout;
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                const int i = (cs + 2 * t) * 32 + lc;
                const bool ok = kv && i < a.din;
                const float w1 = ok ? a.W1[(int64_t)ko * a.din + i] : 0.f;
                const float w2 = ok ? a.W2[(int64_t)ko * a.din + i] : 0.f;
                aS[t] = mfma32(av, w1, aS[t]);
                aT[t] = mfma32(av, w2, aT[t]);
            }
        }
        // phase 3: dE = gprev + dS + dT * X,  dX = dS + dT * E
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const int nb = cs + 2 * t;
            if (nb >= nbi) continue;
            const int i = nb * 32 + lc;
            if (i >= a.din) continue;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int64_t gr = row0 + rb * 32 + mrow(q, lh);
                if (gr >= a.n) continue;
                const float e = a.E[gr * a.lde + i], x = a.X[gr * a.din + i];
                const float gp = a.gprev ? a.gprev[gr * a.ldg + i] : 0.f;
                a.dE[gr * a.din + i] = gp + fmaf(aT[t][q], x, aS[t][q]);
                a.dX[gr * a.din + i] = fmaf(aT[t][q], e, aS[t][q]);
            }
        }
    }
}

struct NgWg {
    const float *dZ, *E;
    int64_t lde;
    const float *X;
    int64_t n, rpc;     // rows, rows per chunk (a multiple of kNgWRows)
    int din, dout;
    float *slab;        // [nchunks][dout][2 din + 1]: dW1 | dW2 | db partials of each chunk
};

// grid (chunks, tile groups): the 32x32 tiles of [dW1 | dW2] (d_out x 2 d_in, each half padded to 32 columns) are
// dealt to the waves, TPW per wave; group 0 also sums db
template <int TPW>
__global__ __launch_bounds__(kBlock) void k_ngcf_wgrad(NgWg a) {
    __shared__ float sZ[kNgWRows][DAISY_NGCF_MAX_WIDTH + 1];
    __shared__ float sST[kNgWRows][2 * DAISY_NGCF_MAX_WIDTH + 1];
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave, lc = lane & 31, lh = lane >> 5;
    const int nbo = (a.dout + 31) / 32, nbi = (a.din + 31) / 32, ntile = nbo * 2 * nbi;
    const int wz = nbo * 32, wst = 2 * nbi * 32;
    const int64_t chunk = blockIdx.x;
    const int64_t r0 = chunk * a.rpc, r1 = min(a.n, r0 + a.rpc);
    const bool do_db = blockIdx.y == 0 && (int)threadIdx.x < a.dout;
    floatx16 acc[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
    float db = 0.f;
    for (int64_t s0 = r0; s0 < r1; s0 += kNgWRows) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < kNgWRows * wz; idx += kBlock) {
            const int r = idx / wz, c = idx % wz;
            const int64_t gr = s0 + r;
            sZ[r][c] = (gr < r1 && c < a.dout) ? a.dZ[gr * a.dout + c] : 0.f;
        }
        for (int idx = threadIdx.x; idx < kNgWRows * wst; idx += kBlock) {
            const int r = idx / wst, c = idx % wst;
            const bool half = c >= nbi * 32;
            const int i = half ? c - nbi * 32 : c;
            const int64_t gr = s0 + r;
            float v = 0.f;
            if (gr < r1 && i < a.din) {
                const float e = a.E[gr * a.lde + i], x = a.X[gr * a.din + i];
                v = half ? x * e : e + x;
            }
            sST[r][c] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kNgWRows; kk += 2) {
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
                const int t = (int)blockIdx.y * 4 * TPW + wave + 4 * j;
                if (t >= ntile) continue;
                const int ob = t / (2 * nbi), cb = t % (2 * nbi);
                acc[j] = mfma32(sZ[kk + lh][ob * 32 + lc], sST[kk + lh][cb * 32 + lc], acc[j]);
            }
        }
        if (do_db)
            for (int r = 0; r < kNgWRows; ++r) db += sZ[r][threadIdx.x];
    }
    const int w = 2 * a.din + 1;
    float *slab = a.slab + chunk * (int64_t)a.dout * w;
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        const int t = (int)blockIdx.y * 4 * TPW + wave + 4 * j;
        if (t >= ntile) continue;
        const int ob = t / (2 * nbi), cb = t % (2 * nbi);
        const int col = cb * 32 + lc;
        const int nc = col < nbi * 32 ? (col < a.din ? col : -1) : (col - nbi * 32 < a.din ? a.din + col - nbi * 32 : -1);
        if (nc < 0) continue;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int o = ob * 32 + mrow(q, lh);
            if (o < a.dout) slab[(int64_t)o * w + nc] = acc[j][q];
        }
    }
    if (do_db) slab[(int64_t)threadIdx.x * w + 2 * a.din] = db;
}

__global__ void k_ngcf_wgrad_sum(const float *__restrict__ slab, int64_t nchunks, int din, int dout,
                                 float *__restrict__ dW1, float *__restrict__ db1, float *__restrict__ dW2,
                                 float *__restrict__ db2) {
    const int w = 2 * din + 1;
    const int64_t total = (int64_t)dout * w;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int64_t c = 0; c < nchunks; ++c) s += slab[c * total + idx];
        const int o = (int)(idx / w), nc = (int)(idx % w);
        if (nc < din) dW1[(int64_t)o * din + nc] += s;
        else if (nc < 2 * din) dW2[(int64_t)o * din + nc - din] += s;
        else { db1[o] += s; db2[o] += s; }
    }
}

__global__ void k_dropout_mask(uint64_t seed, uint32_t stream, int64_t n, uint32_t thresh, uint8_t *__restrict__ out) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
        out[e] = (thresh == 0 || drop_keep(seed, stream, (uint64_t)e, thresh)) ? 1 : 0;
}

// the weight-gradient chunking depends on n only (never on the device), so the summation order is fixed
static int64_t wgrad_rows_per_chunk(int64_t n) {
    int64_t nch = (n + 511) / 512;
    if (nch < 1) nch = 1;
    if (nch > 256) nch = 256;
    int64_t rpc = (n + nch - 1) / nch;
    return (rpc + kNgWRows - 1) / kNgWRows * kNgWRows;
}
static int64_t wgrad_chunks(int64_t n) {
    const int64_t rpc = wgrad_rows_per_chunk(n);
    return (n + rpc - 1) / rpc;
}
static bool width_ok(int32_t d) { return d >= 1 && d <= DAISY_NGCF_MAX_WIDTH; }

}  // namespace daisy

using namespace daisy;


#define NGCF_CHECK_SHAPE(fn, n, d_in, d_out)                                                                     \
    DAISY_CHECK_ARG((n) > 0 && width_ok(d_in) && width_ok(d_out),                                              \
                    fn ": n=%lld d_in=%d d_out=%d (widths 1..%d, n > 0)", (long long)(n), (int)(d_in), (int)(d_out), \
                    DAISY_NGCF_MAX_WIDTH)

extern "C" {

int daisy_dropout_mask(uint64_t seed, uint32_t stream_id, int64_t n, float p, uint8_t *out, daisy_stream_t stream) {
    DAISY_CHECK_ARG(out != nullptr && n > 0, "dropout_mask: NULL output or n <= 0");
    DAISY_CHECK_ARG(p >= 0.f && p < 1.f, "dropout_mask: p=%g outside [0, 1)", (double)p);
    hipLaunchKernelGGL(k_dropout_mask, dim3(grid_for(n, kBlock * 4)), dim3(kBlock), 0, as_stream(stream), seed, stream_id, n,
                       keep_threshold(p), out);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

size_t daisy_ngcf_ws_bytes(int64_t n, int32_t d_in, int32_t d_out) {
    if (n <= 0 || !width_ok(d_in) || !width_ok(d_out)) return 0;
    return align_up((size_t)n * d_out * 4) + (size_t)wgrad_chunks(n) * d_out * (2 * d_in + 1) * 4;
}

int daisy_ngcf_layer_forward(const float *E, int64_t lde, const float *X, const float *W1, const float *b1,
                             const float *W2, const float *b2, float *Y, int64_t ldy, float *norm, int64_t n,
                             int32_t d_in, int32_t d_out, float mess_p, uint64_t seed, int32_t layer,
                             daisy_stream_t stream) {
    NGCF_CHECK_SHAPE("ngcf_layer_forward", n, d_in, d_out);
    DAISY_CHECK_ARG(E && X && W1 && b1 && W2 && b2 && Y && norm, "ngcf_layer_forward: NULL argument");
    DAISY_CHECK_ARG(lde >= d_in && ldy >= d_out, "ngcf_layer_forward: row pitch below the width");
    DAISY_CHECK_ARG(mess_p >= 0.f && mess_p < 1.f, "ngcf_layer_forward: mess_p=%g outside [0, 1)", (double)mess_p);
    DAISY_CHECK_ARG(layer >= 0, "ngcf_layer_forward: layer < 0");
    NgFwd a{E, lde, X, W1, b1, W2, b2, Y, ldy, norm, n, d_in, d_out, keep_threshold(mess_p),
            DAISY_NGCF_MESS_STREAM + (uint32_t)layer, 1.f, seed};
    a.scale = a.thresh ? 1.f / (1.f - mess_p) : 1.f;
    const dim3 grid(grid_for(n, kNgRows)), block(kBlock);
    hipStream_t s = as_stream(stream);
    switch ((d_out + 31) / 32) {
        case 1: hipLaunchKernelGGL(k_ngcf_layer_fwd<1>, grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL(k_ngcf_layer_fwd<2>, grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL(k_ngcf_layer_fwd<3>, grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL(k_ngcf_layer_fwd<4>, grid, block, 0, s, a); break;
        case 5: hipLaunchKernelGGL(k_ngcf_layer_fwd<5>, grid, block, 0, s, a); break;
        case 6: hipLaunchKernelGGL(k_ngcf_layer_fwd<6>, grid, block, 0, s, a); break;
        case 7: hipLaunchKernelGGL(k_ngcf_layer_fwd<7>, grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL(k_ngcf_layer_fwd<8>, grid, block, 0, s, a); break;
    }
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_ngcf_layer_backward(const float *dY, int64_t ldd, const float *Y, int64_t ldy, const float *norm,
                              const float *E, int64_t lde, const float *X, const float *W1, const float *W2,
                              const float *gprev, int64_t ldg, float *dE, float *dX, float *ws, int64_t n,
                              int32_t d_in, int32_t d_out, float mess_p, uint64_t seed, int32_t layer,
                              daisy_stream_t stream) {
    NGCF_CHECK_SHAPE("ngcf_layer_backward", n, d_in, d_out);
    DAISY_CHECK_ARG(dY && Y && norm && E && X && W1 && W2 && dE && dX && ws, "ngcf_layer_backward: NULL argument");
    DAISY_CHECK_ARG(ldd >= d_out && ldy >= d_out && lde >= d_in && (!gprev || ldg >= d_in),
                    "ngcf_layer_backward: row pitch below the width");
    DAISY_CHECK_ARG(dE != dX && (const float *)dE != dY && (const float *)dX != dY,
                    "ngcf_layer_backward: dE, dX and dY must be distinct buffers");
    DAISY_CHECK_ARG(mess_p >= 0.f && mess_p < 1.f, "ngcf_layer_backward: mess_p=%g outside [0, 1)", (double)mess_p);
    DAISY_CHECK_ARG(layer >= 0, "ngcf_layer_backward: layer < 0");
    hipStream_t s = as_stream(stream);
    float *dZ = ws;
    float *slab = (float *)((char *)ws + align_up((size_t)n * d_out * 4));
    NgBwd a{dY, ldd, Y, ldy, norm, E, lde, X, W1, W2, gprev, ldg, dE, dX, dZ, n, d_in, d_out,
            keep_threshold(mess_p), DAISY_NGCF_MESS_STREAM + (uint32_t)layer, 1.f, seed};
    a.scale = a.thresh ? 1.f / (1.f - mess_p) : 1.f;
    const dim3 grid(grid_for(n, kNgBRows)), block(kBlock);
    const int nbi = (d_in + 31) / 32, tpw = (nbi + 1) / 2;
    switch (tpw) {
        case 1: hipLaunchKernelGGL(k_ngcf_layer_bwd<1>, grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL(k_ngcf_layer_bwd<2>, grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL(k_ngcf_layer_bwd<3>, grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL(k_ngcf_layer_bwd<4>, grid, block, 0, s, a); break;
    }
    DAISY_LAUNCH_CHECK();
    NgWg w{dZ, E, lde, X, n, wgrad_rows_per_chunk(n), d_in, d_out, slab};
    const int ntile = ((d_out + 31) / 32) * 2 * nbi;
    const int64_t nch = wgrad_chunks(n);
    auto go = [&](auto kern, int per_wave) {
        hipLaunchKernelGGL(kern, dim3((unsigned)nch, (unsigned)((ntile + 4 * per_wave - 1) / (4 * per_wave))), block, 0,
                           s, w);
    };
    if (ntile <= 4) go(k_ngcf_wgrad<1>, 1);
    else if (ntile <= 8) go(k_ngcf_wgrad<2>, 2);
    else if (ntile <= 16) go(k_ngcf_wgrad<4>, 4);
    else go(k_ngcf_wgrad<8>, 8);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_ngcf_wgrad_reduce(const float *ws, int64_t n, int32_t d_in, int32_t d_out, float *dW1, float *db1,
                            float *dW2, float *db2, daisy_stream_t stream) {
    NGCF_CHECK_SHAPE("ngcf_wgrad_reduce", n, d_in, d_out);
    DAISY_CHECK_ARG(ws && dW1 && db1 && dW2 && db2, "ngcf_wgrad_reduce: NULL argument");
    const float *slab = (const float *)((const char *)ws + align_up((size_t)n * d_out * 4));
    const int64_t total = (int64_t)d_out * (2 * d_in + 1);
    hipLaunchKernelGGL(k_ngcf_wgrad_sum, dim3(grid_for(total, kBlock)), dim3(kBlock), 0, as_stream(stream), slab,
                       wgrad_chunks(n), (int)d_in, (int)d_out, dW1, db1, dW2, db2);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // extern "C"
