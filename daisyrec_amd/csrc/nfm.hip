// NFM (daisy/model/NFMRecommender.py:15-209) on gfx950, fp32 like the reference.
//
// A step is the reference's calc_loss + backward over R = 2B rows (pairwise: the positives' forward call on rows
// 0..B-1, the negatives' on rows B..2B-1) or R = B rows (point-wise).  Stage s = 0..L of the MLP holds its
// pre-normalisation activations Z_s [R][d]:
//     Z_0 = P[u] * Q[i]                 k_nfm_gather            (+ per-tile column partials, + regulariser partials)
//     Z_s = H_{s-1} W_s^T + b_s         k_nfm_linear            H_{s-1} = drop(act(BN(Z_{s-1}))) applied on load
//     BN statistics of each call        k_nfm_bn_stats          the tiles' fp64 partials summed in tile order
//     pred = (H_L + ub + ib + bias) . wp, criterion            k_nfm_head, k_nfm_loss
// and the backward pass per stage, L .. 0:
//     dY = act' * drop' * dH            k_nfm_bwd_act           (+ per-tile column partials of dY, dY * xhat)
//     dZ = BN backward of each call     k_nfm_bn_bwd_stats + k_nfm_bn_bwd_apply
//     dH_{s-1} = dZ W_s                 k_nfm_linear (transposed weight)
//     dW_s, db_s                        k_nfm_wgrad + k_nfm_wgrad_sum (chunk partials summed in chunk order)
//     dP, dQ, d ub, d ib (stage 0)      ids sorted by a stable radix sort, every run summed in row order by its head
// No float atomics touch a result: two runs of a step give the same bits.  Rows of one workgroup tile never straddle
// the two calls, so every per-call column reduction is a sum over whole tiles.
#include "common.h"
#include "pairs.h"

namespace daisy {

constexpr int kNfTR = 32;                   // rows per tile
constexpr int kNfLd = DAISY_NFM_MAX_FACTORS + 1;
constexpr int kNfWChunks = 64;              // most row chunks of the weight-gradient partials
constexpr int kNfWOut = 16;                 // weight-gradient outputs per thread and chunk
constexpr float kNfEps = 1e-5f, kNfMomentum = 0.1f;

// what a stage applies to its Z before the next stage reads it
struct NfStage {
    const float *Z;                  // [R][d]
    const float *mean, *istd;        // [ncalls][d] (batch statistics) or NULL: running statistics below
    const float *rmean, *rvar;       // running statistics (eval mode)
    const float *gamma, *beta;       // BN affine (NULL: no BN)
    int act;                         // DAISY_NFM_ACT_* (stage 0: none)
    uint32_t thresh;                 // dropout (0: off)
    float scale;
    uint32_t stream;
};

__device__ __forceinline__ float nf_act(int act, float y) {
    if (act == DAISY_NFM_ACT_RELU) return y > 0.f ? y : 0.f;
    if (act == DAISY_NFM_ACT_SIGMOID) return 1.f / (1.f + expf(-y));
    if (act == DAISY_NFM_ACT_TANH) return tanhf(y);
    return y;
}
// d act / d y from y and a = act(y)
__device__ __forceinline__ float nf_act_grad(int act, float y, float a) {
    if (act == DAISY_NFM_ACT_RELU) return y > 0.f ? 1.f : 0.f;
    if (act == DAISY_NFM_ACT_SIGMOID) return a * (1.f - a);
    if (act == DAISY_NFM_ACT_TANH) return 1.f - a * a;
    return 1.f;
}

__device__ __forceinline__ void nf_bn_coef(const NfStage &st, int call, int d, int c, float &m, float &is) {
    if (st.mean) {
        m = st.mean[call * d + c];
        is = st.istd[call * d + c];
    } else {
        m = st.rmean[c];
        is = 1.f / sqrtf(st.rvar[c] + kNfEps);
    }
}

// H = drop(act(BN(z))) of element (row r of call `call`, column c); y: the BN output, a: the activation
__device__ __forceinline__ float nf_apply(const NfStage &st, int call, int64_t r, int d, int c, float z, uint64_t seed,
                                          float *y_out = nullptr, float *a_out = nullptr) {
    float y = z;
    if (st.gamma) {
        float m, is;
        nf_bn_coef(st, call, d, c, m, is);
        y = (z - m) * is * st.gamma[c] + st.beta[c];
    }
    const float a = nf_act(st.act, y);
    if (y_out) *y_out = y;
    if (a_out) *a_out = a;
    if (st.thresh && !drop_keep(seed, st.stream, (uint64_t)r * (uint64_t)d + (uint64_t)c, st.thresh)) return 0.f;
    return st.thresh ? a * st.scale : a;
}

struct NfTiles {
    int64_t Bc;         // rows per call
    int64_t tpc;        // tiles per call
    __device__ __forceinline__ void tile(int64_t t, int &call, int64_t &r0, int &rows) const {
        call = (int)(t / tpc);
        const int64_t lo = (t % tpc) * kNfTR;
        r0 = call * Bc + lo;
        rows = (int)((Bc - lo < kNfTR) ? Bc - lo : kNfTR);
    }
};

// a [kNfTR][ld] tile of LDS (ld = d + 1: conflict-free column walks)
struct NfT {
    float *p;
    int ld;
    __device__ __forceinline__ float &operator()(int r, int c) const { return p[r * ld + c]; }
};
// the LDS of every phase: two tiles and 2 048 doubles (sized by d at launch: nf_lds_bytes)
struct NfLds {
    float *base;
    int ld;
    __device__ __forceinline__ NfT a() const { return NfT{base, ld}; }
    __device__ __forceinline__ NfT b() const { return NfT{base + kNfTR * ld, ld}; }
    __device__ __forceinline__ double *x() const { return reinterpret_cast<double *>(base + 2 * kNfTR * ld); }
};
extern __shared__ double nf_lds_dyn[];
// (every kernel that takes LDS is launched with nf_lds_bytes(d) of dynamic LDS; its d is the pitch less one)
__device__ __forceinline__ NfLds nf_lds_for(int d) { return NfLds{reinterpret_cast<float *>(nf_lds_dyn), d + 1}; }
inline size_t nf_lds_bytes(int d) { return (size_t)2 * kNfTR * (d + 1) * 4 + (size_t)kBlock * 4 * 8; }

// per-column fp64 sums of a [rows][d] LDS tile (and of the squares) into part[t][0..d) / [d..2d)
__device__ __forceinline__ void nf_tile_colsums(NfT s, int rows, int d, double *part) {
    for (int c = threadIdx.x; c < d; c += blockDim.x) {
        double s1 = 0.0, s2 = 0.0;
        for (int r = 0; r < rows; ++r) {
            const double v = s(r, c);
            s1 += v;
            s2 += v * v;
        }
        part[c] = s1;
        part[d + c] = s2;
    }
}

// Z_0 = P[u] * Q[i]; per tile: column sums (BN) and the regulariser sums (sum |x|, sum x^2 of the gathered user and item rows)
__device__ __forceinline__ void nf_gather(const float *__restrict__ P, const float *__restrict__ Q, PairSrc src,
                                                       NfTiles tl, int64_t ntiles, int d, float *__restrict__ Z,
                                                       double *__restrict__ part, double *__restrict__ regpart, NfLds lds) {
    const NfT sZ = lds.a();
    double *sR = lds.x();
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int call, rows;
        int64_t r0;
        tl.tile(t, call, r0, rows);
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        for (int idx = threadIdx.x; idx < rows * d; idx += blockDim.x) {
            const int r = idx / d, c = idx % d;
            int64_t user, item;
            pair_ids(src, r0 + r, user, item);
            const float p = P[user * d + c], q = Q[item * d + c];
            const float z = p * q;
            Z[(r0 + r) * d + c] = z;
            sZ(r, c) = z;
            a[0] += fabs((double)p);
            a[1] += (double)p * p;
            a[2] += fabs((double)q);
            a[3] += (double)q * q;
        }
        for (int k = 0; k < 4; ++k) sR[threadIdx.x * 4 + k] = a[k];
        __syncthreads();
        if (part) nf_tile_colsums(sZ, rows, d, part + t * 2 * d);
        if (regpart && threadIdx.x < 4) {
            double s = 0.0;
            for (int k = 0; k < (int)blockDim.x; ++k) s += sR[k * 4 + threadIdx.x];
            regpart[t * 4 + threadIdx.x] = s;
        }
        __syncthreads();
    }
}
__global__ __launch_bounds__(kBlock) void k_nfm_gather(const float *__restrict__ P, const float *__restrict__ Q, PairSrc src,
                                                       NfTiles tl, int64_t ntiles, int d, float *__restrict__ Z,
                                                       double *__restrict__ part, double *__restrict__ regpart) { nf_gather(P, Q, src, tl, ntiles, d, Z, part, regpart, nf_lds_for(d)); }

// Out[r][c] = bias[c] + sum_k H[r][k] * W(c, k) over a tile; W(c, k) = W[c * d + k] (forward) or W[k * d + c] (trans: the
// input gradient dZ W).  H is stage `in`'s output (in.Z transformed) or, with in.Z == NULL, Hraw as it is.
__device__ __forceinline__ void nf_linear(NfStage in, const float *__restrict__ Hraw, const float *__restrict__ W,
                                                       const float *__restrict__ bias, int trans, NfTiles tl, int64_t ntiles,
                                                       int d, uint64_t seed, float *__restrict__ Out, double *__restrict__ part, NfLds lds) {
    const NfT sH = lds.a(), sO = lds.b();
    const int64_t wc = trans ? 1 : d, wk = trans ? d : 1;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int call, rows;
        int64_t r0;
        tl.tile(t, call, r0, rows);
        for (int idx = threadIdx.x; idx < rows * d; idx += blockDim.x) {
            const int r = idx / d, c = idx % d;
            const int64_t gr = r0 + r;
            sH(r, c) = in.Z ? nf_apply(in, call, gr, d, c, in.Z[gr * d + c], seed) : Hraw[gr * d + c];
        }
        __syncthreads();
        // column-major outputs: the lanes of a half wave share the weight element and read 32 consecutive rows of LDS
        for (int idx = threadIdx.x; idx < kNfTR * d; idx += blockDim.x) {
            const int c = idx / kNfTR, r = idx % kNfTR;
            if (r >= rows) continue;
            const float *w = W + c * wc;
            float acc = bias ? bias[c] : 0.f;
            for (int k = 0; k < d; ++k) acc = fmaf(sH(r, k), w[k * wk], acc);
            sO(r, c) = acc;
            Out[(r0 + r) * d + c] = acc;
        }
        __syncthreads();
        if (part) nf_tile_colsums(sO, rows, d, part + t * 2 * d);
        __syncthreads();
    }
}
__global__ __launch_bounds__(kBlock) void k_nfm_linear(NfStage in, const float *__restrict__ Hraw, const float *__restrict__ W,
                                                       const float *__restrict__ bias, int trans, NfTiles tl, int64_t ntiles,
                                                       int d, uint64_t seed, float *__restrict__ Out, double *__restrict__ part) { nf_linear(in, Hraw, W, bias, trans, tl, ntiles, d, seed, Out, part, nf_lds_for(d)); }

// batch statistics of one stage: per call and column, the tiles' partial sums in tile order (fp64); mean, 1/sqrt(var + eps)
// (biased variance) for the normalisation, the running statistics updated call after call (unbiased variance)
__device__ __forceinline__ void nf_bn_stats(const double *__restrict__ part, int ncalls, int64_t tpc, int64_t Bc,
                                                         int d, float *__restrict__ mean, float *__restrict__ istd,
                                                         float *__restrict__ rmean, float *__restrict__ rvar,
                                                         int64_t *__restrict__ nbt) {
    for (int c = threadIdx.x; c < d; c += blockDim.x) {
        for (int call = 0; call < ncalls; ++call) {
            double s1 = 0.0, s2 = 0.0;
            for (int64_t t = call * tpc; t < (call + 1) * tpc; ++t) {
                s1 += part[t * 2 * d + c];
                s2 += part[t * 2 * d + d + c];
            }
            const double n = (double)Bc, m = s1 / n;
            double var = s2 / n - m * m;
            if (var < 0.0) var = 0.0;
            mean[call * d + c] = (float)m;
            istd[call * d + c] = (float)(1.0 / sqrt(var + (double)kNfEps));
            if (rmean) {
                const float unb = (float)(n > 1.0 ? var * n / (n - 1.0) : var);
                rmean[c] = (1.f - kNfMomentum) * rmean[c] + kNfMomentum * (float)m;
                rvar[c] = (1.f - kNfMomentum) * rvar[c] + kNfMomentum * unb;
            }
        }
    }
    if (nbt && threadIdx.x == 0 && blockIdx.x == 0) nbt[0] += ncalls;
}
__global__ __launch_bounds__(kBlock) void k_nfm_bn_stats(const double *__restrict__ part, int ncalls, int64_t tpc, int64_t Bc,
                                                         int d, float *__restrict__ mean, float *__restrict__ istd,
                                                         float *__restrict__ rmean, float *__restrict__ rvar,
                                                         int64_t *__restrict__ nbt) { nf_bn_stats(part, ncalls, tpc, Bc, d, mean, istd, rmean, rvar, nbt); }

// pred[r] = sum_c (H_L[r][c] + ub[u] + ib[i] + bias) * wp[c]
__device__ __forceinline__ void nf_head(NfStage st, const float *__restrict__ ub, const float *__restrict__ ib,
                                                     const float *__restrict__ bias, const float *__restrict__ wp, PairSrc src,
                                                     int64_t R, int64_t Bc, int d, uint64_t seed, float *__restrict__ pred) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x) {
        int64_t user, item;
        pair_ids(src, r, user, item);
        const int call = (int)(r / Bc);
        const float bs = ub[user] + ib[item] + bias[0];
        float s = 0.f;
        for (int c = 0; c < d; ++c) s = fmaf(nf_apply(st, call, r, d, c, st.Z[r * d + c], seed) + bs, wp[c], s);
        pred[r] = s;
    }
}
__global__ __launch_bounds__(kBlock) void k_nfm_head(NfStage st, const float *__restrict__ ub, const float *__restrict__ ib,
                                                     const float *__restrict__ bias, const float *__restrict__ wp, PairSrc src,
                                                     int64_t R, int64_t Bc, int d, uint64_t seed, float *__restrict__ pred) { nf_head(st, ub, ib, bias, wp, src, R, Bc, d, seed, pred); }

__device__ __noinline__ void nf_loss_tail(const double *sm, int pointwise, const double *__restrict__ regpart, int64_t tpc,
                                          float reg_1, float reg_2, double *__restrict__ stats);
// criterion + regulariser (one workgroup, fixed order): dpred, stats[LOSS_DATA, NORM_*, LOSS], stats[LOSS_SUM] +=
__device__ __forceinline__ void nf_loss(const float *__restrict__ pred, const int32_t *__restrict__ j, int64_t B,
                                                     int loss_type, float gamma, int pointwise, const double *__restrict__ regpart,
                                                     int64_t tpc, float reg_1, float reg_2, float *__restrict__ dpred,
                                                     double *__restrict__ stats, NfLds lds) {
    double *sm = lds.x();
    double acc = 0.0;
    for (int64_t b = threadIdx.x; b < B; b += blockDim.x) {
        float term, cp, cn;
        pair_coef(loss_type, pred[b], pointwise ? (float)j[b] : pred[B + b], gamma, term, cp, cn);
        dpred[b] = cp;
        if (!pointwise) dpred[B + b] = cn;
        acc += (double)term;
    }
    sm[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) nf_loss_tail(sm, pointwise, regpart, tpc, reg_1, reg_2, stats);
}
__global__ __launch_bounds__(kBlock) void k_nfm_loss(const float *__restrict__ pred, const int32_t *__restrict__ j, int64_t B,
                                                     int loss_type, float gamma, int pointwise, const double *__restrict__ regpart,
                                                     int64_t tpc, float reg_1, float reg_2, float *__restrict__ dpred,
                                                     double *__restrict__ stats) { nf_loss(pred, j, B, loss_type, gamma, pointwise, regpart, tpc, reg_1, reg_2, dpred, stats, nf_lds_for(0)); }

__device__ __noinline__ void nf_loss_tail(const double *sm, int pointwise, const double *__restrict__ regpart, int64_t tpc,
                                          float reg_1, float reg_2, double *__restrict__ stats) {
    double loss = 0.0;
    for (int k = 0; k < (int)blockDim.x; ++k) loss += sm[k];
    stats[DAISY_NFM_ST_LOSS_DATA] = loss;
    double l1[3] = {0.0, 0.0, 0.0}, sq[3] = {0.0, 0.0, 0.0};   // user rows (first call), items of call 0, items of call 1
    if (regpart) {
        const int ncalls = pointwise ? 1 : 2;
        for (int call = 0; call < ncalls; ++call)
            for (int64_t t = call * tpc; t < (call + 1) * tpc; ++t) {
                if (call == 0) {
                    l1[0] += regpart[t * 4 + 0];
                    sq[0] += regpart[t * 4 + 1];
                }
                l1[1 + call] += regpart[t * 4 + 2];
                sq[1 + call] += regpart[t * 4 + 3];
            }
    }
    double reg = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double n = sqrt(sq[k]);
        stats[DAISY_NFM_ST_NORM_U + k] = n;
        reg += (double)reg_1 * l1[k] + (double)reg_2 * n;
    }
    loss += reg;
    stats[DAISY_NFM_ST_LOSS] = loss;
    stats[DAISY_NFM_ST_LOSS_SUM] += loss;
    if (!(fabs(loss) <= 1.7976931348623157e308)) stats[DAISY_NFM_ST_NONFINITE] += 1.0;
}

// dH_L = dpred * wp; per row d(ub + ib) = dpred * sum(wp); per tile: d wp partials and d bias
__device__ __forceinline__ void nf_head_bwd(NfStage st, const float *__restrict__ ub, const float *__restrict__ ib,
                                                         const float *__restrict__ bias, const float *__restrict__ wp,
                                                         PairSrc src, NfTiles tl, int64_t ntiles, int d, uint64_t seed,
                                                         const float *__restrict__ dpred, float *__restrict__ G,
                                                         float *__restrict__ dbs, float *__restrict__ wpart, NfLds lds) {
    const NfT sT = lds.a();
    float *sB = lds.b().p, *sD = sB + kNfTR;
    float swp = 0.f;
    for (int c = 0; c < d; ++c) swp += wp[c];
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int call, rows;
        int64_t r0;
        tl.tile(t, call, r0, rows);
        for (int r = threadIdx.x; r < rows; r += blockDim.x) {
            int64_t user, item;
            pair_ids(src, r0 + r, user, item);
            sB[r] = ub[user] + ib[item] + bias[0];
            sD[r] = dpred[r0 + r];
            dbs[r0 + r] = dpred[r0 + r] * swp;
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < rows * d; idx += blockDim.x) {
            const int r = idx / d, c = idx % d;
            const int64_t gr = r0 + r;
            const float h = nf_apply(st, call, gr, d, c, st.Z[gr * d + c], seed);
            sT(r, c) = sD[r] * (h + sB[r]);
            G[gr * d + c] = sD[r] * wp[c];
        }
        __syncthreads();
        for (int c = threadIdx.x; c <= d; c += blockDim.x) {
            float s = 0.f;
            if (c < d)
                for (int r = 0; r < rows; ++r) s += sT(r, c);
            else
                for (int r = 0; r < rows; ++r) s += sD[r] * swp;
            wpart[t * (d + 1) + c] = s;
        }
        __syncthreads();
    }
}
__global__ __launch_bounds__(kBlock) void k_nfm_head_bwd(NfStage st, const float *__restrict__ ub, const float *__restrict__ ib,
                                                         const float *__restrict__ bias, const float *__restrict__ wp,
                                                         PairSrc src, NfTiles tl, int64_t ntiles, int d, uint64_t seed,
                                                         const float *__restrict__ dpred, float *__restrict__ G,
                                                         float *__restrict__ dbs, float *__restrict__ wpart) { nf_head_bwd(st, ub, ib, bias, wp, src, tl, ntiles, d, seed, dpred, G, dbs, wpart, nf_lds_for(d)); }

// d wp[c] += sum over tiles (tile order); d bias += the tiles' sums of the rows' d(ub + ib), each call's sum on its own and then
// the two added, as autograd adds the two forward calls' gradients (under BPR / HL they cancel exactly, as in the reference)
__device__ __forceinline__ void nf_head_sum(const float *__restrict__ wpart, int ncalls, int64_t tpc, int d,
                                                         float *__restrict__ gwp, float *__restrict__ gbias) {
    for (int c = threadIdx.x; c <= d; c += blockDim.x) {
        float s = 0.f;
        for (int call = 0; call < ncalls; ++call) {
            float sc = 0.f;
            for (int64_t t = call * tpc; t < (call + 1) * tpc; ++t) sc += wpart[t * (d + 1) + c];
            s += sc;
        }
        if (c < d) gwp[c] += s;
        else gbias[0] += s;
    }
}
__global__ __launch_bounds__(kBlock) void k_nfm_head_sum(const float *__restrict__ wpart, int ncalls, int64_t tpc, int d,
                                                         float *__restrict__ gwp, float *__restrict__ gbias) { nf_head_sum(wpart, ncalls, tpc, d, gwp, gbias); }

// dY = act'(y) * drop'(dH) in place of G; with BN, per tile the column sums of dY and dY * xhat
__device__ __forceinline__ void nf_bwd_act(NfStage st, NfTiles tl, int64_t ntiles, int d, uint64_t seed,
                                                        float *__restrict__ G, double *__restrict__ part, NfLds lds) {
    const NfT sY = lds.a(), sX = lds.b();
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int call, rows;
        int64_t r0;
        tl.tile(t, call, r0, rows);
        for (int idx = threadIdx.x; idx < rows * d; idx += blockDim.x) {
            const int r = idx / d, c = idx % d;
            const int64_t gr = r0 + r;
            const float z = st.Z[gr * d + c];
            float y, a;
            const float h = nf_apply(st, call, gr, d, c, z, seed, &y, &a);
            float g = G[gr * d + c];
            (void)h;
            if (st.thresh)
                g = drop_keep(seed, st.stream, (uint64_t)gr * (uint64_t)d + (uint64_t)c, st.thresh) ? g * st.scale : 0.f;
            g *= nf_act_grad(st.act, y, a);
            G[gr * d + c] = g;
            if (part) {
                float m, is;
                nf_bn_coef(st, call, d, c, m, is);
                sY(r, c) = g;
                sX(r, c) = g * ((z - m) * is);
            }
        }
        if (!part) continue;
        __syncthreads();
        for (int c = threadIdx.x; c < d; c += blockDim.x) {
            double s1 = 0.0, s2 = 0.0;
            for (int r = 0; r < rows; ++r) {
                s1 += (double)sY(r, c);
                s2 += (double)sX(r, c);
            }
            part[t * 2 * d + c] = s1;
            part[t * 2 * d + d + c] = s2;
        }
        __syncthreads();
    }
}
__global__ __launch_bounds__(kBlock) void k_nfm_bwd_act(NfStage st, NfTiles tl, int64_t ntiles, int d, uint64_t seed,
                                                        float *__restrict__ G, double *__restrict__ part) { nf_bwd_act(st, tl, ntiles, d, seed, G, part, nf_lds_for(d)); }

// per call and column: k1 = mean dY, k2 = mean dY * xhat (tile order); d beta += sum dY, d gamma += sum dY * xhat (call order)
__device__ __forceinline__ void nf_bn_bwd_stats(const double *__restrict__ part, int ncalls, int64_t tpc, int64_t Bc,
                                                             int d, float *__restrict__ k12, float *__restrict__ ggamma,
                                                             float *__restrict__ gbeta) {
    for (int c = threadIdx.x; c < d; c += blockDim.x) {
        double gb = 0.0, gg = 0.0;
        for (int call = 0; call < ncalls; ++call) {
            double s1 = 0.0, s2 = 0.0;
            for (int64_t t = call * tpc; t < (call + 1) * tpc; ++t) {
                s1 += part[t * 2 * d + c];
                s2 += part[t * 2 * d + d + c];
            }
            k12[call * 2 * d + c] = (float)(s1 / (double)Bc);
            k12[call * 2 * d + d + c] = (float)(s2 / (double)Bc);
            gb += s1;
            gg += s2;
        }
        gbeta[c] += (float)gb;
        ggamma[c] += (float)gg;
    }
}
__global__ __launch_bounds__(kBlock) void k_nfm_bn_bwd_stats(const double *__restrict__ part, int ncalls, int64_t tpc, int64_t Bc,
                                                             int d, float *__restrict__ k12, float *__restrict__ ggamma,
                                                             float *__restrict__ gbeta) { nf_bn_bwd_stats(part, ncalls, tpc, Bc, d, k12, ggamma, gbeta); }

// dZ = gamma * istd * (dY - k1 - xhat * k2) in place
__device__ __forceinline__ void nf_bn_bwd_apply(NfStage st, const float *__restrict__ k12, int64_t R, int64_t Bc,
                                                             int d, float *__restrict__ G) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < R * d; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = e / d;
        const int c = (int)(e % d), call = (int)(r / Bc);
        float m, is;
        nf_bn_coef(st, call, d, c, m, is);
        const float xh = (st.Z[e] - m) * is;
        G[e] = st.gamma[c] * is * (G[e] - k12[call * 2 * d + c] - xh * k12[call * 2 * d + d + c]);
    }
}
__global__ __launch_bounds__(kBlock) void k_nfm_bn_bwd_apply(NfStage st, const float *__restrict__ k12, int64_t R, int64_t Bc,
                                                             int d, float *__restrict__ G) { nf_bn_bwd_apply(st, k12, R, Bc, d, G); }

// weight gradient partials of row chunk blockIdx.x: ws[chunk][c * d + k] = sum_r dZ[r][c] H[r][k], ws[chunk][d*d + c] = sum_r dZ[r][c];
// blockIdx.y: the group of kBlock * kNfWOut outputs.  H = stage `in` applied to its Z.
__device__ __forceinline__ void nf_wgrad(NfStage in, const float *__restrict__ G, int64_t R, int64_t Bc,
                                                      int64_t rpc, int d, uint64_t seed, float *__restrict__ ws, int chunk,
                                                      int group, NfLds lds) {
    const NfT sG = lds.a(), sH = lds.b();
    const int64_t nout = (int64_t)d * d + d;
    const int64_t o0 = (int64_t)group * kBlock * kNfWOut;
    float acc[kNfWOut];
#pragma unroll
    for (int q = 0; q < kNfWOut; ++q) acc[q] = 0.f;
    const int64_t lo = chunk * rpc, hi = (lo + rpc < R) ? lo + rpc : R;
    for (int64_t r0 = lo; r0 < hi; r0 += kNfTR) {
        const int rows = (int)((hi - r0 < kNfTR) ? hi - r0 : kNfTR);
        __syncthreads();
        for (int idx = threadIdx.x; idx < rows * d; idx += blockDim.x) {
            const int r = idx / d, c = idx % d;
            const int64_t gr = r0 + r;
            sG(r, c) = G[gr * d + c];
            sH(r, c) = nf_apply(in, (int)(gr / Bc), gr, d, c, in.Z[gr * d + c], seed);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kNfWOut; ++q) {
            const int64_t o = o0 + q * kBlock + threadIdx.x;
            if (o >= nout) continue;
            const int c = (o < (int64_t)d * d) ? (int)(o / d) : (int)(o - (int64_t)d * d);
            const int k = (o < (int64_t)d * d) ? (int)(o % d) : -1;
            float s = acc[q];
            for (int r = 0; r < rows; ++r) s = fmaf(sG(r, c), k >= 0 ? sH(r, k) : 1.f, s);
            acc[q] = s;
        }
    }
#pragma unroll
    for (int q = 0; q < kNfWOut; ++q) {
        const int64_t o = o0 + q * kBlock + threadIdx.x;
        if (o < nout) ws[chunk * nout + o] = acc[q];
    }
}
__global__ __launch_bounds__(kBlock) void k_nfm_wgrad(NfStage in, const float *__restrict__ G, int64_t R, int64_t Bc,
                                                      int64_t rpc, int d, uint64_t seed, float *__restrict__ ws) { nf_wgrad(in, G, R, Bc, rpc, d, seed, ws, (int)blockIdx.x, (int)blockIdx.y, nf_lds_for(d)); }

// dW, db += the chunks' partials in chunk order
__device__ __forceinline__ void nf_wgrad_sum(const float *__restrict__ ws, int nchunks, int d, float *__restrict__ gW,
                                                          float *__restrict__ gb) {
    const int64_t nout = (int64_t)d * d + d;
    for (int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; o < nout; o += (int64_t)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int k = 0; k < nchunks; ++k) s += ws[k * nout + o];
        if (o < (int64_t)d * d) gW[o] += s;
        else gb[o - (int64_t)d * d] += s;
    }
}
__global__ __launch_bounds__(kBlock) void k_nfm_wgrad_sum(const float *__restrict__ ws, int nchunks, int d, float *__restrict__ gW,
                                                          float *__restrict__ gb) { nf_wgrad_sum(ws, nchunks, d, gW, gb); }

// sort keys: the user (side 0) or item (side 1) id of every row, values the row
__device__ __forceinline__ void nf_keys(PairSrc src, int64_t R, int side, int32_t *__restrict__ key, int32_t *__restrict__ val) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x) {
        int64_t user, item;
        pair_ids(src, r, user, item);
        key[r] = (int32_t)(side ? item : user);
        val[r] = (int32_t)r;
    }
}
__global__ __launch_bounds__(kBlock) void k_nfm_keys(PairSrc src, int64_t R, int side, int32_t *__restrict__ key, int32_t *__restrict__ val) { nf_keys(src, R, side, key, val); }

// embedding gradient of one side: the head of every run of equal ids sums its rows in row order (the sort is stable) and
// adds the sum to the gradient row once.  Column d is the bias embedding.  Side 0 (users): dZ0 * Q[item] + the regulariser
// of the rows of the first call; side 1 (items): dZ0 * P[user] + the regulariser of the call's item norm.
__device__ __forceinline__ void nf_embed_grad(const int32_t *__restrict__ key, const int32_t *__restrict__ val, int64_t R,
                                                           int side, PairSrc src, int64_t Bc, int d, const float *__restrict__ P,
                                                           const float *__restrict__ Q, const float *__restrict__ G,
                                                           const float *__restrict__ dbs, float reg_1, float reg_2,
                                                           const double *__restrict__ stats, float *__restrict__ gT,
                                                           float *__restrict__ gbias) {
    const int64_t n = R * (int64_t)(d + 1);
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = e / (d + 1);
        const int c = (int)(e % (d + 1));
        const int32_t id = key[p];
        if (p > 0 && key[p - 1] == id) continue;
        const float *own = side ? Q : P;
        float nrm[2] = {0.f, 0.f};
        if (reg_2 != 0.f) {
            nrm[0] = (float)stats[side ? DAISY_NFM_ST_NORM_I : DAISY_NFM_ST_NORM_U];
            nrm[1] = (float)stats[DAISY_NFM_ST_NORM_J];
        }
        const float x = (c < d) ? own[(int64_t)id * d + c] : 0.f;
        const float sg = (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f);
        // each call's rows summed on their own, then the two sums added (autograd's order: the rows come sorted by row,
        // so the first call's rows precede the second's)
        float acc = 0.f, acc0 = 0.f;
        bool second = false;
        for (int64_t q = p; q < R && key[q] == id; ++q) {
            const int64_t r = val[q];
            if (!second && r >= Bc) {
                second = true;
                acc0 = acc;
                acc = 0.f;
            }
            if (c == d) {
                acc += dbs[r];
                continue;
            }
            int64_t user, item;
            pair_ids(src, r, user, item);
            const float other = side ? P[user * d + c] : Q[item * d + c];
            acc = fmaf(G[r * d + c], other, acc);
            const int call = (int)(r / Bc);
            if (side == 0 && call != 0) continue;        // the regulariser takes every user row once (the first call)
            const float nr = nrm[side ? call : 0];
            acc += reg_1 * sg + (nr > 0.f ? reg_2 * x / nr : 0.f);
        }
        if (second) acc = acc0 + acc;
        if (c < d) gT[(int64_t)id * d + c] += acc;
        else gbias[id] += acc;
    }
}
__global__ __launch_bounds__(kBlock) void k_nfm_embed_grad(const int32_t *__restrict__ key, const int32_t *__restrict__ val, int64_t R,
                                                           int side, PairSrc src, int64_t Bc, int d, const float *__restrict__ P,
                                                           const float *__restrict__ Q, const float *__restrict__ G,
                                                           const float *__restrict__ dbs, float reg_1, float reg_2,
                                                           const double *__restrict__ stats, float *__restrict__ gT,
                                                           float *__restrict__ gbias) { nf_embed_grad(key, val, R, side, src, Bc, d, P, Q, G, dbs, reg_1, reg_2, stats, gT, gbias); }

// One training step: everything daisy_nfm_step_grads hands to the kernels of either path.
struct NfStep {
    PairSrc src;
    const int32_t *j;
    int64_t B, R, tpc, ntiles, rpc;
    int ncalls, nch, d, L, bn, reg, pointwise, loss_type;
    float gamma, reg_1, reg_2;
    uint64_t seed;
    NfStage st[DAISY_NFM_MAX_LAYERS + 1];
    const float *P, *Q, *ub, *ib, *bias, *wp, *W[DAISY_NFM_MAX_LAYERS], *b[DAISY_NFM_MAX_LAYERS];
    float *gP, *gQ, *gub, *gib, *gbias, *gwp, *gW[DAISY_NFM_MAX_LAYERS], *gb[DAISY_NFM_MAX_LAYERS];
    float *gbn_w[DAISY_NFM_MAX_LAYERS + 1], *gbn_b[DAISY_NFM_MAX_LAYERS + 1];
    float *rmean[DAISY_NFM_MAX_LAYERS + 1], *rvar[DAISY_NFM_MAX_LAYERS + 1];
    int64_t *nbt[DAISY_NFM_MAX_LAYERS + 1];
    float *Z, *G, *G2, *pred, *dpred, *dbs, *stat, *k12, *wpart, *wws;
    double *part, *regpart, *stats;
    int32_t *kout, *vout;
};

// The small step (B <= DAISY_NFM_SMALL_MAX_B): the whole step in ONE workgroup - the phases of the layered path, in the same
// order and with the same tiles and chunks, separated by barriers instead of launches, so both paths give the same bits.  The
// stable sort of the embedding-gradient rows is a rank count in LDS.
__global__ __launch_bounds__(kBlock) void k_nfm_small_step(NfStep a) {
    const NfLds lds = nf_lds_for(a.d);
    const NfTiles tl{a.B, a.tpc};
    const int d = a.d, L = a.L;
    double *part = a.bn ? a.part : nullptr;
    nf_gather(a.P, a.Q, a.src, tl, a.ntiles, d, a.Z, part, a.reg ? a.regpart : nullptr, lds);
    __syncthreads();
    for (int k = 0; k <= L; ++k) {
        if (k > 0) {
            nf_linear(a.st[k - 1], nullptr, a.W[k - 1], a.b[k - 1], 0, tl, a.ntiles, d, a.seed, a.Z + (int64_t)k * a.R * d, part, lds);
            __syncthreads();
        }
        if (a.bn) {
            nf_bn_stats(a.part, a.ncalls, a.tpc, a.B, d, a.stat + (int64_t)k * 4 * d, a.stat + (int64_t)k * 4 * d + 2 * d, a.rmean[k],
                        a.rvar[k], a.nbt[k]);
            __syncthreads();
        }
    }
    nf_head(a.st[L], a.ub, a.ib, a.bias, a.wp, a.src, a.R, a.B, d, a.seed, a.pred);
    __syncthreads();
    nf_loss(a.pred, a.j, a.B, a.loss_type, a.gamma, a.pointwise, a.reg ? a.regpart : nullptr, a.tpc, a.reg_1, a.reg_2, a.dpred,
            a.stats, nf_lds_for(0));
    __syncthreads();
    float *G = a.G, *G2 = a.G2;
    nf_head_bwd(a.st[L], a.ub, a.ib, a.bias, a.wp, a.src, tl, a.ntiles, d, a.seed, a.dpred, G, a.dbs, a.wpart, lds);
    __syncthreads();
    nf_head_sum(a.wpart, a.ncalls, a.tpc, d, a.gwp, a.gbias);
    __syncthreads();
    const int64_t nout = (int64_t)d * d + d;
    const int ngroups = (int)((nout + kBlock * kNfWOut - 1) / (kBlock * kNfWOut));
    for (int k = L; k >= 0; --k) {
        nf_bwd_act(a.st[k], tl, a.ntiles, d, a.seed, G, part, lds);
        __syncthreads();
        if (a.bn) {
            nf_bn_bwd_stats(a.part, a.ncalls, a.tpc, a.B, d, a.k12, a.gbn_w[k], a.gbn_b[k]);
            __syncthreads();
            nf_bn_bwd_apply(a.st[k], a.k12, a.R, a.B, d, G);
            __syncthreads();
        }
        if (k == 0) break;
        for (int chunk = 0; chunk < a.nch; ++chunk)
            for (int group = 0; group < ngroups; ++group) {
                nf_wgrad(a.st[k - 1], G, a.R, a.B, a.rpc, d, a.seed, a.wws, chunk, group, lds);
                __syncthreads();
            }
        nf_wgrad_sum(a.wws, a.nch, d, a.gW[k - 1], a.gb[k - 1]);
        __syncthreads();
        NfStage raw{};
        nf_linear(raw, G, a.W[k - 1], nullptr, 1, tl, a.ntiles, d, a.seed, G2, nullptr, lds);
        __syncthreads();
        float *tmp = G;
        G = G2;
        G2 = tmp;
    }
    int32_t *key = reinterpret_cast<int32_t *>(lds.x());        // R <= 2 * DAISY_NFM_SMALL_MAX_B ids
    for (int side = 0; side < 2; ++side) {
        for (int64_t r = threadIdx.x; r < a.R; r += blockDim.x) {
            int64_t user, item;
            pair_ids(a.src, r, user, item);
            key[r] = (int32_t)(side ? item : user);
        }
        __syncthreads();
        // stable sort by rank: position of row r = rows with a smaller id + rows before r with the same id
        for (int64_t r = threadIdx.x; r < a.R; r += blockDim.x) {
            const int32_t kr = key[r];
            int pos = 0;
            for (int64_t q = 0; q < a.R; ++q) {
                const int32_t kq = key[q];
                pos += (kq < kr) || (kq == kr && q < r);
            }
            a.kout[pos] = kr;
            a.vout[pos] = (int32_t)r;
        }
        __syncthreads();
        nf_embed_grad(a.kout, a.vout, a.R, side, a.src, a.B, d, a.P, a.Q, G, a.dbs, a.reg_1, a.reg_2, a.stats, side ? a.gQ : a.gP,
                      side ? a.gib : a.gub);
        __syncthreads();
    }
}

// eval-mode score of every pair: gather, the L affine BN / act / Linear stages, bias, the prediction dot (one workgroup per tile
// of rows, activations in LDS)
struct NfEval {
    const float *P, *Q, *ub, *ib, *bias, *wp;
    const float *W[DAISY_NFM_MAX_LAYERS], *b[DAISY_NFM_MAX_LAYERS];
    const float *gamma[DAISY_NFM_MAX_LAYERS + 1], *beta[DAISY_NFM_MAX_LAYERS + 1];
    const float *rmean[DAISY_NFM_MAX_LAYERS + 1], *rvar[DAISY_NFM_MAX_LAYERS + 1];
    int L, d, act;
};
__device__ __forceinline__ float nf_eval_post(const NfEval &a, int s, int c, float z) {
    if (a.gamma[s]) z = (z - a.rmean[s][c]) * (1.f / sqrtf(a.rvar[s][c] + kNfEps)) * a.gamma[s][c] + a.beta[s][c];
    return s ? nf_act(a.act, z) : z;
}
__global__ __launch_bounds__(kBlock) void k_nfm_scores(NfEval a, PairSrc src, int64_t n, float *__restrict__ out) {
    __shared__ float sH[2][kNfTR][kNfLd];
    const int d = a.d;
    const int64_t ntiles = (n + kNfTR - 1) / kNfTR;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t r0 = t * kNfTR;
        const int rows = (int)((n - r0 < kNfTR) ? n - r0 : kNfTR);
        __syncthreads();
        for (int idx = threadIdx.x; idx < rows * d; idx += blockDim.x) {
            const int r = idx / d, c = idx % d;
            int64_t user, item;
            pair_ids(src, r0 + r, user, item);
            sH[0][r][c] = nf_eval_post(a, 0, c, a.P[user * d + c] * a.Q[item * d + c]);
        }
        int cur = 0;
        for (int l = 1; l <= a.L; ++l) {
            __syncthreads();
            const float *W = a.W[l - 1];
            for (int idx = threadIdx.x; idx < kNfTR * d; idx += blockDim.x) {
                const int c = idx / kNfTR, r = idx % kNfTR;
                if (r >= rows) continue;
                float acc = a.b[l - 1][c];
                for (int k = 0; k < d; ++k) acc = fmaf(sH[cur][r][k], W[(int64_t)c * d + k], acc);
                sH[cur ^ 1][r][c] = nf_eval_post(a, l, c, acc);
            }
            cur ^= 1;
        }
        __syncthreads();
        // one 32-lane group per row: the dot over the columns, halved in lane order
        const int lane = threadIdx.x & 31, grp = threadIdx.x >> 5;
        for (int r = grp; r < rows; r += kBlock / 32) {
            int64_t user, item;
            pair_ids(src, r0 + r, user, item);
            const float bs = a.ub[user] + a.ib[item] + a.bias[0];
            float s = 0.f;
            for (int c = lane; c < d; c += 32) s = fmaf(sH[cur][r][c] + bs, a.wp[c], s);
            for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off, 32);
            if (lane == 0) out[r0 + r] = s;
        }
    }
}

}  // namespace daisy

using namespace daisy;

struct daisy_nfm_ctx {
    int64_t max_rows;    // rows of one forward call
    int d, L, act, bn;
    int64_t user_num, item_num;
    DeviceArena arena;
    float *Z, *G, *G2, *pred, *dpred, *dbs, *stat, *k12, *wpart, *wws;
    double *part, *regpart;
    int32_t *kin, *kout, *vin, *vout;
    void *sort_tmp;
    size_t sort_bytes;
    int path = DAISY_NFM_PATH_AUTO;
};

namespace {

int64_t nf_tiles_per_call(int64_t Bc) { return (Bc + kNfTR - 1) / kNfTR; }
int64_t nf_wchunk_rows(int64_t R) {
    int64_t rpc = (R + kNfWChunks - 1) / kNfWChunks;
    return (rpc + kNfTR - 1) / kNfTR * kNfTR;
}

NfStage nf_stage(const daisy_nfm_ctx *c, const daisy_nfm_params *p, const daisy_nfm_bn_state *bn, int s, int64_t R, bool batch_stats,
                 uint32_t thresh, float scale) {
    NfStage st{};
    st.Z = c->Z + (int64_t)s * R * c->d;
    if (c->bn) {
        st.gamma = p->bn_w[s];
        st.beta = p->bn_b[s];
        if (batch_stats) {
            st.mean = c->stat + (int64_t)s * 4 * c->d;
            st.istd = st.mean + 2 * c->d;
        } else {
            st.rmean = bn->mean[s];
            st.rvar = bn->var[s];
        }
    }
    st.act = s ? c->act : DAISY_NFM_ACT_NONE;
    st.thresh = thresh;
    st.scale = scale;
    st.stream = DAISY_NFM_DROP_STREAM + (uint32_t)s;
    return st;
}

// the training-mode forward of every stage over R = ncalls * Bc rows (batch statistics, running statistics updated)
int nf_forward(daisy_nfm_ctx *c, const daisy_nfm_params *p, const daisy_nfm_bn_state *bn, const PairSrc &src, int ncalls,
               int64_t Bc, bool reg, uint32_t thresh, float scale, uint64_t seed, NfStage *st, hipStream_t s) {
    const int d = c->d;
    const int64_t R = ncalls * Bc, tpc = nf_tiles_per_call(Bc), ntiles = ncalls * tpc;
    const NfTiles tl{Bc, tpc};
    for (int k = 0; k <= c->L; ++k) st[k] = nf_stage(c, p, bn, k, R, true, thresh, scale);
    const int grid = grid_for(ntiles, 1);
    hipLaunchKernelGGL(k_nfm_gather, dim3(grid), dim3(kBlock), nf_lds_bytes(d), s, p->P, p->Q, src, tl, ntiles, d, c->Z,
                       c->bn ? c->part : nullptr, reg ? c->regpart : nullptr);
    DAISY_LAUNCH_CHECK();
    for (int k = 0; k <= c->L; ++k) {
        if (k > 0) {
            hipLaunchKernelGGL(k_nfm_linear, dim3(grid), dim3(kBlock), nf_lds_bytes(d), s, st[k - 1], (const float *)nullptr, p->W[k - 1], p->b[k - 1],
                               0, tl, ntiles, d, seed, c->Z + (int64_t)k * R * d, c->bn ? c->part : nullptr);
            DAISY_LAUNCH_CHECK();
        }
        if (c->bn) {
            hipLaunchKernelGGL(k_nfm_bn_stats, dim3(1), dim3(kBlock), 0, s, c->part, ncalls, tpc, Bc, d, c->stat + (int64_t)k * 4 * d,
                               c->stat + (int64_t)k * 4 * d + 2 * d, bn->mean[k], bn->var[k], bn->nbt[k]);
            DAISY_LAUNCH_CHECK();
        }
    }
    return DAISY_OK;
}

int nf_check_params(const daisy_nfm_ctx *c, const daisy_nfm_params *p, const char *what) {
    DAISY_CHECK_ARG(p->P && p->Q && p->ub && p->ib && p->bias && p->wp, "%s: null embedding / bias / prediction pointer", what);
    for (int l = 0; l < c->L; ++l) DAISY_CHECK_ARG(p->W[l] && p->b[l], "%s: null weight of layer %d", what, l + 1);
    if (c->bn)
        for (int s = 0; s <= c->L; ++s) DAISY_CHECK_ARG(p->bn_w[s] && p->bn_b[s], "%s: null BatchNorm affine of stage %d", what, s);
    return DAISY_OK;
}

// train: the running statistics are updated (num_batches_tracked needed too)
int nf_check_bn(const daisy_nfm_ctx *c, const daisy_nfm_bn_state *bn, const char *what, bool train = true) {
    if (!c->bn) return DAISY_OK;
    DAISY_CHECK_ARG(bn != nullptr, "%s: batch_norm needs the running statistics", what);
    for (int s = 0; s <= c->L; ++s)
        DAISY_CHECK_ARG(bn->mean[s] && bn->var[s] && (bn->nbt[s] || !train), "%s: null running statistics of stage %d", what, s);
    return DAISY_OK;
}

// the eval-mode launch daisy_nfm_scores and daisy_nfm_scores_users share
int nf_scores_eval(daisy_nfm_ctx *ctx, const daisy_nfm_params *params, const daisy_nfm_bn_state *bn, const PairSrc &src,
                          int64_t n, float *out, hipStream_t s) {
    NfEval a{};
    a.P = params->P;
    a.Q = params->Q;
    a.ub = params->ub;
    a.ib = params->ib;
    a.bias = params->bias;
    a.wp = params->wp;
    for (int l = 0; l < ctx->L; ++l) {
        a.W[l] = params->W[l];
        a.b[l] = params->b[l];
    }
    for (int k = 0; k <= ctx->L; ++k)
        if (ctx->bn) {
            a.gamma[k] = params->bn_w[k];
            a.beta[k] = params->bn_b[k];
            a.rmean[k] = bn->mean[k];
            a.rvar[k] = bn->var[k];
        }
    a.L = ctx->L;
    a.d = ctx->d;
    a.act = ctx->act;
    hipLaunchKernelGGL(k_nfm_scores, dim3(grid_for((n + kNfTR - 1) / kNfTR, 1, 4096)), dim3(kBlock), 0, s, a, src, n, out);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // namespace

extern "C" {

int daisy_nfm_ctx_create(daisy_nfm_ctx **out, int64_t max_rows, int32_t factors, int32_t num_layers, int32_t act,
                         int32_t batch_norm, int64_t user_num, int64_t item_num) {
    DAISY_CHECK_ARG(out, "nfm_ctx_create: out is NULL");
    *out = nullptr;
    DAISY_CHECK_ARG(max_rows >= 1 && max_rows <= (1ll << 26), "nfm_ctx_create: max_rows=%lld (1 .. 2^26)", (long long)max_rows);
    DAISY_CHECK_ARG(factors >= 1 && factors <= DAISY_NFM_MAX_FACTORS, "nfm_ctx_create: factors=%d (1 .. %d)", factors,
                    DAISY_NFM_MAX_FACTORS);
    DAISY_CHECK_ARG(num_layers >= 0 && num_layers <= DAISY_NFM_MAX_LAYERS, "nfm_ctx_create: num_layers=%d (0 .. %d)", num_layers,
                    DAISY_NFM_MAX_LAYERS);
    DAISY_CHECK_ARG(act >= DAISY_NFM_ACT_NONE && act <= DAISY_NFM_ACT_TANH, "nfm_ctx_create: act=%d", act);
    DAISY_CHECK_ARG(user_num >= 1 && item_num >= 1 && user_num < (1ll << 31) && item_num < (1ll << 31),
                    "nfm_ctx_create: user_num=%lld item_num=%lld", (long long)user_num, (long long)item_num);
    daisy_nfm_ctx *c = new daisy_nfm_ctx();
    c->max_rows = max_rows;
    c->d = factors;
    c->L = num_layers;
    c->act = act;
    c->bn = batch_norm != 0;
    c->user_num = user_num;
    c->item_num = item_num;
    const int64_t R = 2 * max_rows, d = factors, T = 2 * nf_tiles_per_call(max_rows);
    const int64_t nch = kNfWChunks;         // (the chunk count of a step is at most this, not monotonic in R)
    c->sort_bytes = sort_pairs_i32_temp_bytes_upto(R);
    DeviceArena &a = c->arena;
    a.add(&c->Z, (size_t)(c->L + 1) * R * d * 4); a.add(&c->G, (size_t)R * d * 4); a.add(&c->G2, (size_t)R * d * 4);
    a.add(&c->pred, R * 4); a.add(&c->dpred, R * 4); a.add(&c->dbs, R * 4);
    a.add(&c->stat, (size_t)(c->L + 1) * 4 * d * 4); a.add(&c->k12, 4 * d * 4);
    a.add(&c->wpart, (size_t)T * (d + 1) * 4); a.add(&c->wws, (size_t)nch * (d * d + d) * 4);
    a.add(&c->part, (size_t)T * 2 * d * 8); a.add(&c->regpart, (size_t)T * 4 * 8);
    a.add(&c->kin, R * 4); a.add(&c->kout, R * 4); a.add(&c->vin, R * 4); a.add(&c->vout, R * 4);
    a.add(&c->sort_tmp, c->sort_bytes);
    if (int rc = a.alloc("nfm_ctx_create")) {
        delete c;
        return rc;
    }
    const int lds = (int)nf_lds_bytes(factors);
    const void *lds_kernels[] = {(const void *)k_nfm_gather, (const void *)k_nfm_linear, (const void *)k_nfm_head_bwd,
                                 (const void *)k_nfm_bwd_act, (const void *)k_nfm_wgrad, (const void *)k_nfm_small_step};
    for (const void *kf : lds_kernels) {
        const hipError_t e = hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) {
            c->arena.release();
            delete c;
            set_error("nfm_ctx_create: hipFuncSetAttribute(%d B of LDS) failed: %s", lds, hipGetErrorString(e));
            return DAISY_ERR_HIP;
        }
    }
    *out = c;
    return DAISY_OK;
}

int daisy_nfm_ctx_destroy(daisy_nfm_ctx *ctx) {
    if (!ctx) return DAISY_OK;
    ctx->arena.release();
    delete ctx;
    return DAISY_OK;
}

size_t daisy_nfm_ctx_bytes(const daisy_nfm_ctx *ctx) { return ctx ? ctx->arena.bytes() : 0; }

int daisy_nfm_ctx_set_path(daisy_nfm_ctx *ctx, int32_t path) {
    DAISY_CHECK_ARG(ctx, "nfm_ctx_set_path: ctx is NULL");
    DAISY_CHECK_ARG(path >= DAISY_NFM_PATH_AUTO && path <= DAISY_NFM_PATH_LAYERED, "nfm_ctx_set_path: path=%d (0 auto, 1 small, 2 layered)",
                    path);
    ctx->path = path;
    return DAISY_OK;
}

int daisy_nfm_step_grads(daisy_nfm_ctx *ctx, const daisy_nfm_params *params, const daisy_nfm_params *grads,
                         const daisy_nfm_bn_state *bn, const int32_t *u, const int32_t *i, const int32_t *j, int64_t B,
                         int32_t loss_type, float gamma, float reg_1, float reg_2, float dropout_p, uint64_t seed,
                         double *stats, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && params && grads && u && i && j && stats, "nfm_step_grads: null argument");
    DAISY_CHECK_ARG(B >= 1 && B <= ctx->max_rows, "nfm_step_grads: B=%lld (1 .. %lld)", (long long)B, (long long)ctx->max_rows);
    DAISY_CHECK_ARG(loss_type >= DAISY_LOSS_BPR && loss_type <= DAISY_LOSS_SL, "nfm_step_grads: loss_type=%d", loss_type);
    DAISY_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "nfm_step_grads: dropout=%g (0 <= p < 1)", (double)dropout_p);
    DAISY_CHECK_ARG(!ctx->bn || B > 1, "nfm_step_grads: Expected more than 1 value per channel when training (BatchNorm, B=1)");
    DAISY_CHECK_ARG(ctx->path != DAISY_NFM_PATH_SMALL || B <= DAISY_NFM_SMALL_MAX_B,
                    "nfm_step_grads: the small path takes B <= %d (B=%lld)", DAISY_NFM_SMALL_MAX_B, (long long)B);
    if (int rc = nf_check_params(ctx, params, "nfm_step_grads")) return rc;
    if (int rc = nf_check_params(ctx, grads, "nfm_step_grads (grads)")) return rc;
    if (int rc = nf_check_bn(ctx, bn, "nfm_step_grads")) return rc;
    hipStream_t s = as_stream(stream);
    const daisy_nfm_params &p = *params, &g = *grads;
    const int d = ctx->d, L = ctx->L;
    NfStep a{};
    a.pointwise = (loss_type == DAISY_LOSS_CL || loss_type == DAISY_LOSS_SL);
    a.ncalls = a.pointwise ? 1 : 2;
    a.B = B;
    a.R = a.ncalls * B;
    a.tpc = nf_tiles_per_call(B);
    a.ntiles = a.ncalls * a.tpc;
    a.rpc = nf_wchunk_rows(a.R);
    a.nch = (int)((a.R + a.rpc - 1) / a.rpc);
    a.d = d;
    a.L = L;
    a.bn = ctx->bn;
    a.reg = reg_1 != 0.f || reg_2 != 0.f;
    a.loss_type = loss_type;
    a.gamma = gamma;
    a.reg_1 = reg_1;
    a.reg_2 = reg_2;
    a.seed = seed;
    a.src.u = u;
    a.src.i = i;
    a.src.j = a.pointwise ? i : j;
    a.src.B = B;
    a.j = j;
    const uint32_t thresh = keep_threshold(dropout_p);
    const float scale = thresh ? 1.f / (1.f - dropout_p) : 1.f;
    for (int k = 0; k <= L; ++k) {
        a.st[k] = nf_stage(ctx, &p, bn, k, a.R, true, thresh, scale);
        if (ctx->bn) {
            a.gbn_w[k] = g.bn_w[k];
            a.gbn_b[k] = g.bn_b[k];
            a.rmean[k] = bn->mean[k];
            a.rvar[k] = bn->var[k];
            a.nbt[k] = bn->nbt[k];
        }
    }
    a.P = p.P; a.Q = p.Q; a.ub = p.ub; a.ib = p.ib; a.bias = p.bias; a.wp = p.wp;
    a.gP = g.P; a.gQ = g.Q; a.gub = g.ub; a.gib = g.ib; a.gbias = g.bias; a.gwp = g.wp;
    for (int l = 0; l < L; ++l) {
        a.W[l] = p.W[l];
        a.b[l] = p.b[l];
        a.gW[l] = g.W[l];
        a.gb[l] = g.b[l];
    }
    a.Z = ctx->Z; a.G = ctx->G; a.G2 = ctx->G2; a.pred = ctx->pred; a.dpred = ctx->dpred; a.dbs = ctx->dbs;
    a.stat = ctx->stat; a.k12 = ctx->k12; a.wpart = ctx->wpart; a.wws = ctx->wws; a.part = ctx->part; a.regpart = ctx->regpart;
    a.stats = stats; a.kout = ctx->kout; a.vout = ctx->vout;
    const size_t lds = nf_lds_bytes(d);
    if (ctx->path == DAISY_NFM_PATH_SMALL) {     // (auto: the layered path - see DESIGN.md §13 for why)
        hipLaunchKernelGGL(k_nfm_small_step, dim3(1), dim3(kBlock), lds, s, a);
        DAISY_LAUNCH_CHECK();
        return DAISY_OK;
    }
    // the layered path: every phase a launch over all tiles
    if (int rc = nf_forward(ctx, &p, bn, a.src, a.ncalls, B, a.reg, thresh, scale, seed, a.st, s)) return rc;
    const int64_t R = a.R, tpc = a.tpc, ntiles = a.ntiles;
    const int ncalls = a.ncalls;
    const NfTiles tl{B, tpc};
    const int grid = grid_for(ntiles, 1);
    NfStage *st = a.st;
    hipLaunchKernelGGL(k_nfm_head, dim3(grid_for(R, kBlock)), dim3(kBlock), 0, s, st[L], p.ub, p.ib, p.bias, p.wp, a.src, R, B, d,
                       seed, ctx->pred);
    DAISY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_nfm_loss, dim3(1), dim3(kBlock), nf_lds_bytes(0), s, ctx->pred, j, B, loss_type, gamma, a.pointwise,
                       a.reg ? ctx->regpart : nullptr, tpc, reg_1, reg_2, ctx->dpred, stats);
    DAISY_LAUNCH_CHECK();
    float *G = ctx->G, *G2 = ctx->G2;
    hipLaunchKernelGGL(k_nfm_head_bwd, dim3(grid), dim3(kBlock), lds, s, st[L], p.ub, p.ib, p.bias, p.wp, a.src, tl, ntiles, d, seed,
                       ctx->dpred, G, ctx->dbs, ctx->wpart);
    DAISY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_nfm_head_sum, dim3(1), dim3(kBlock), 0, s, ctx->wpart, ncalls, tpc, d, g.wp, g.bias);
    DAISY_LAUNCH_CHECK();
    double *part = ctx->bn ? ctx->part : nullptr;
    for (int k = L; k >= 0; --k) {
        hipLaunchKernelGGL(k_nfm_bwd_act, dim3(grid), dim3(kBlock), lds, s, st[k], tl, ntiles, d, seed, G, part);
        DAISY_LAUNCH_CHECK();
        if (ctx->bn) {
            hipLaunchKernelGGL(k_nfm_bn_bwd_stats, dim3(1), dim3(kBlock), 0, s, ctx->part, ncalls, tpc, B, d, ctx->k12, g.bn_w[k],
                               g.bn_b[k]);
            DAISY_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_nfm_bn_bwd_apply, dim3(grid_for(R * d, kBlock)), dim3(kBlock), 0, s, st[k], ctx->k12, R, B, d, G);
            DAISY_LAUNCH_CHECK();
        }
        if (k == 0) break;
        const int64_t nout = (int64_t)d * d + d;
        hipLaunchKernelGGL(k_nfm_wgrad, dim3(a.nch, (unsigned)((nout + kBlock * kNfWOut - 1) / (kBlock * kNfWOut))), dim3(kBlock), lds,
                           s, st[k - 1], G, R, B, a.rpc, d, seed, ctx->wws);
        DAISY_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_nfm_wgrad_sum, dim3(grid_for(nout, kBlock)), dim3(kBlock), 0, s, ctx->wws, a.nch, d, g.W[k - 1],
                           g.b[k - 1]);
        DAISY_LAUNCH_CHECK();
        NfStage raw{};
        hipLaunchKernelGGL(k_nfm_linear, dim3(grid), dim3(kBlock), lds, s, raw, G, p.W[k - 1], (const float *)nullptr, 1, tl, ntiles,
                           d, seed, G2, (double *)nullptr);
        DAISY_LAUNCH_CHECK();
        float *tmp = G;
        G = G2;
        G2 = tmp;
    }
    // stage 0: dZ_0 (in G) to the embedding rows, per side through a stable sort of the rows by id
    for (int side = 0; side < 2; ++side) {
        hipLaunchKernelGGL(k_nfm_keys, dim3(grid_for(R, kBlock)), dim3(kBlock), 0, s, a.src, R, side, ctx->kin, ctx->vin);
        DAISY_LAUNCH_CHECK();
        const int64_t rows = side ? ctx->item_num : ctx->user_num;
        if (int rc = sort_pairs_i32(ctx->sort_tmp, ctx->sort_bytes, ctx->kin, ctx->kout, ctx->vin, ctx->vout, R, bits_for(rows), s))
            return rc;
        hipLaunchKernelGGL(k_nfm_embed_grad, dim3(grid_for(R * (d + 1), kBlock, kMaxGridSparse)), dim3(kBlock), 0, s, ctx->kout,
                           ctx->vout, R, side, a.src, B, d, p.P, p.Q, G, ctx->dbs, reg_1, reg_2, stats, side ? g.Q : g.P,
                           side ? g.ib : g.ub);
        DAISY_LAUNCH_CHECK();
    }
    return DAISY_OK;
}

int daisy_nfm_fit_epoch(daisy_nfm_ctx *ctx, const daisy_nfm_params *params, const daisy_nfm_params *grads,
                        const daisy_nfm_bn_state *bn, const int32_t *u, const int32_t *i, const int32_t *j, int64_t n,
                        int64_t batch, int32_t loss_type, float gamma, float reg_1, float reg_2, float dropout_p,
                        uint64_t seed_hi, int64_t step0, int64_t opt_step0, int32_t optimizer, float lr, float *W, float *g,
                        float *state0, float *state1, int64_t n_flat, double *stats, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && params && grads && u && i && j && stats && W && g && n > 0 && batch > 0 && n_flat > 0 && step0 >= 0 &&
                    opt_step0 >= 0, "nfm_fit_epoch: bad argument");
    if (int rc = dense_opt_check("nfm_fit_epoch", optimizer, state0, state1)) return rc;
    DAISY_CHECK_ARG(batch <= ctx->max_rows, "nfm_fit_epoch: batch=%lld > max_rows=%lld", (long long)batch, (long long)ctx->max_rows);
    DAISY_CHECK_ARG(!ctx->bn || n % batch != 1,
                    "nfm_fit_epoch: Expected more than 1 value per channel when training (BatchNorm, last batch of 1 row)");
    int64_t step = step0, t = opt_step0;
    for (int64_t s0 = 0; s0 < n; s0 += batch) {
        const int64_t B = (n - s0 < batch) ? n - s0 : batch;
        ++step;
        ++t;
        int rc = daisy_nfm_step_grads(ctx, params, grads, bn, u + s0, i + s0, j + s0, B, loss_type, gamma, reg_1, reg_2, dropout_p,
                                      seed_hi | (uint64_t)step, stats, stream);
        if (rc) return rc;
        if ((rc = dense_opt_step(optimizer, W, g, state0, state1, n_flat, lr, t, stream))) return rc;
    }
    return DAISY_OK;
}

int daisy_nfm_scores(daisy_nfm_ctx *ctx, const daisy_nfm_params *params, const daisy_nfm_bn_state *bn, const int64_t *users,
                     const int64_t *items, int64_t n, int64_t C, int32_t train, float dropout_p, uint64_t seed, float *out,
                     daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && params && users && out, "nfm_scores: null argument");
    DAISY_CHECK_ARG(n >= 1, "nfm_scores: n=%lld", (long long)n);
    DAISY_CHECK_ARG(C >= 0 && (C == 0 || (items && n % C == 0)), "nfm_scores: C=%lld does not divide n=%lld", (long long)C,
                    (long long)n);
    DAISY_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "nfm_scores: dropout=%g (0 <= p < 1)", (double)dropout_p);
    if (int rc = nf_check_params(ctx, params, "nfm_scores")) return rc;
    if (int rc = nf_check_bn(ctx, bn, "nfm_scores", train != 0)) return rc;
    hipStream_t s = as_stream(stream);
    PairSrc src{};
    src.users = users;
    src.items = items;
    src.C = C;
    if (train) {
        // nn.Module in training mode: batch statistics over all n rows (one running-statistics update), dropout acts
        DAISY_CHECK_ARG(n <= ctx->max_rows, "nfm_scores: train-mode n=%lld > max_rows=%lld", (long long)n, (long long)ctx->max_rows);
        DAISY_CHECK_ARG(!ctx->bn || n > 1, "nfm_scores: Expected more than 1 value per channel when training (BatchNorm, n=1)");
        const uint32_t thresh = keep_threshold(dropout_p);
        const float scale = thresh ? 1.f / (1.f - dropout_p) : 1.f;
        NfStage st[DAISY_NFM_MAX_LAYERS + 1];
        if (int rc = nf_forward(ctx, params, bn, src, 1, n, false, thresh, scale, seed, st, s)) return rc;
        hipLaunchKernelGGL(k_nfm_head, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, st[ctx->L], params->ub, params->ib, params->bias,
                           params->wp, src, n, n, ctx->d, seed, out);
        DAISY_LAUNCH_CHECK();
        return DAISY_OK;
    }
    return nf_scores_eval(ctx, params, bn, src, n, out, s);
}

int daisy_nfm_scores_users(daisy_nfm_ctx *ctx, const daisy_nfm_params *params, const daisy_nfm_bn_state *bn,
                           const int64_t *users, int64_t m, float *out, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && params && users && out, "nfm_scores_users: null argument");
    DAISY_CHECK_ARG(m >= 1 && m <= INT64_MAX / ctx->item_num, "nfm_scores_users: m=%lld users (x %lld items)", (long long)m,
                    (long long)ctx->item_num);
    if (int rc = nf_check_params(ctx, params, "nfm_scores_users")) return rc;
    if (int rc = nf_check_bn(ctx, bn, "nfm_scores_users", false)) return rc;
    PairSrc src{};
    src.users = users;
    src.all_items = ctx->item_num;
    return nf_scores_eval(ctx, params, bn, src, m * ctx->item_num, out, as_stream(stream));
}

}  // extern "C"
