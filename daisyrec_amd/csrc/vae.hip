// Multi-VAE (daisy/model/VAECFRecommender.py, VAECF) on gfx950, fp32 like the reference.
//
// A step of B users (their history rows: E CSR entries in all) runs these phases, each over its tiles in a fixed order:
//   k_vae_offsets    the rows' entry offsets in the batch (an exclusive scan)
//   k_vae_prep       per row: 1 / max(||R_b||, 1e-12), the keep bit of every entry
//                    (caller's byte or the counter hash), coef_e = r_e / denom_b * keep_e / (1 - p)
//   k_vae_enc0       the encoder's first layer as a sparse product: h1_b = tanh(b0 + sum_e coef_e W0T[item_e]) with W0T
//                    the item-major copy of encoder.0.weight (one whole row per entry); no dense B x I input
//   vae_linear       every dense layer: fp32 MFMA tiles (gemm_f32), split-k slices summed in slice order + bias + tanh
//   k_vae_reparam    mu | logvar of the reference's index split (odd lat: the middle column unused), z = mu + eps * std,
//                    per row the KL sum (fp64)
//   (decoder)        dense layers; the last one writes the logits [B][I] without its bias
//   k_vae_softmax    per row: online max / sum-exp over the I logits (+ bias) in a fixed tree -> lse_b,
//                    CE_b = s_b * lse_b - sum_{e in R_b} r_e z_e, then dZ = (softmax * s_b - R) / B in place
//   k_vae_loss       one workgroup: CE and KL summed in a fixed order (fp64) -> stats
// and backward: db_out (column sums: row chunks in order), dW_out = dZ^T H, dH = dZ W_out (split-k), tanh', the
// reparameterisation + KL gradients, the dense encoder layers, then dW0T from the kept entries only: the batch's
// entries sorted by item (stable radix sort), every run summed in batch order by its head.  No float atomics.
#include "common.h"
#include "gemm.h"

namespace daisy {

constexpr int kVaeTargetTiles = 256;         // split-k of a product until it has about this many workgroups

// N(0, 1) by Box-Muller from two hashes of the element's counter
__device__ __forceinline__ float vae_normal(uint64_t seed, uint64_t idx) {
    const uint32_t h1 = counter_hash(seed, DAISY_VAE_EPS_STREAM, 2 * idx),
                   h2 = counter_hash(seed, DAISY_VAE_EPS_STREAM, 2 * idx + 1);
    const float u1 = (float)((h1 >> 8) + 1u) * (1.0f / 16777216.0f);        // (0, 1]
    const float u2 = (float)(h2 >> 8) * (1.0f / 16777216.0f);               // [0, 1)
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

// fixed-tree sum over the workgroup (every thread gets the result)
__device__ __forceinline__ double vae_block_sum(double v, double *sm) {
    __syncthreads();
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    const double r = sm[0];
    __syncthreads();
    return r;
}

struct VaeBatch {
    const int64_t *row_ptr;
    const int32_t *col;
    const float *val;
    int64_t user_num;
    const int64_t *users;
    int64_t B, n_entries, item_num;
    const uint8_t *keep;
    uint32_t thresh;             // dropout keep threshold (0: no dropout)
    float scale;                 // 1 / (1 - p)
    int train;
    uint64_t seed;
};

__device__ __forceinline__ int64_t vae_row_len(const VaeBatch &a, int64_t r) {
    const int64_t u = a.users[r];
    if (u < 0 || u >= a.user_num) return 0;
    return a.row_ptr[u + 1] - a.row_ptr[u];
}

// row_off[b] = the entries of rows 0 .. b-1 (an exclusive scan, one workgroup: contiguous runs per thread, the 256 run
// totals scanned in LDS)
__global__ __launch_bounds__(kBlock) void k_vae_offsets(VaeBatch a, int64_t *__restrict__ row_off) {
    __shared__ int64_t part[kBlock];
    const int64_t per = (a.B + kBlock - 1) / kBlock, r0 = threadIdx.x * per, r1 = (r0 + per < a.B) ? r0 + per : a.B;
    int64_t s = 0;
    for (int64_t r = r0; r < r1; ++r) s += vae_row_len(a, r);
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int k = 0; k < kBlock; ++k) {
            const int64_t t = part[k];
            part[k] = run;
            run += t;
        }
    }
    __syncthreads();
    int64_t o = part[threadIdx.x];
    for (int64_t r = r0; r < r1; ++r) {
        row_off[r] = o;
        o += vae_row_len(a, r);
    }
}

// per row b: the norm and the coefficients of its entries (offset row_off[b]).  Out: ent_item / ent_row / ent_idx /
// ent_coef / ent_val [n_entries], row_len / row_bad [B], rsum [B] (sum of R_b).  A row whose entries would pass
// n_entries (a caller count below the real one) is flagged and left empty; the first such row, or the last row when the
// count is above the real one, fills the rest of [0, n_entries) with the sentinel item `item_num`: every entry the
// sort reads is defined.
__global__ __launch_bounds__(kBlock) void k_vae_prep(VaeBatch a, int32_t *__restrict__ ent_item, int32_t *__restrict__ ent_row,
                                                     int32_t *__restrict__ ent_idx, float *__restrict__ ent_coef,
                                                     float *__restrict__ ent_val, const int64_t *__restrict__ row_off,
                                                     int32_t *__restrict__ row_len, double *__restrict__ rsum,
                                                     int32_t *__restrict__ row_bad) {
    __shared__ double sm[kBlock];
    const int64_t b = blockIdx.x;
    const int64_t off = row_off[b];
    const int64_t u = a.users[b];
    const bool bad_id = (u < 0 || u >= a.user_num);
    int64_t len = bad_id ? 0 : a.row_ptr[u + 1] - a.row_ptr[u];
    const bool over = off + len > a.n_entries;
    if (over) len = 0;
    const int64_t lo = bad_id ? 0 : a.row_ptr[u];
    double ss = 0.0, s1 = 0.0;
    for (int64_t e = threadIdx.x; e < len; e += blockDim.x) {
        const float v = a.val[lo + e];
        ss += (double)v * v;
        s1 += (double)v;
    }
    const double sq = vae_block_sum(ss, sm);
    const double sr = vae_block_sum(s1, sm);
    const float denom = fmaxf(sqrtf((float)sq), 1e-12f);
    if (threadIdx.x == 0) {
        row_len[b] = (int32_t)len;
        rsum[b] = sr;
        row_bad[b] = (bad_id || over) ? 1 : 0;
    }
    for (int64_t e = threadIdx.x; e < len; e += blockDim.x) {
        const int64_t x = off + e;
        const float v = a.val[lo + e];
        const float h = v / denom;                        // F.normalize: x / max(||x||, eps)
        bool kept = true;
        if (a.train && a.thresh) kept = a.keep ? (a.keep[x] != 0) : drop_keep(a.seed, DAISY_VAE_KEEP_STREAM, (uint64_t)x, a.thresh);
        ent_item[x] = a.col[lo + e];
        ent_row[x] = (int32_t)b;
        ent_idx[x] = (int32_t)x;
        ent_val[x] = v;
        ent_coef[x] = (a.train && a.thresh) ? (kept ? h * a.scale : 0.f) : h;
    }
    int64_t pad = -1;
    if (over && off < a.n_entries) pad = off;                 // the first row past the count (offsets only grow)
    else if (!over && b == a.B - 1) pad = off + len;
    if (pad >= 0)
        for (int64_t x = pad + threadIdx.x; x < a.n_entries; x += blockDim.x) {
            ent_item[x] = (int32_t)a.item_num;
            ent_row[x] = -1;
            ent_idx[x] = (int32_t)x;
            ent_val[x] = 0.f;
            ent_coef[x] = 0.f;
        }
}

constexpr int kVaeCols = 4;            // columns per thread of the entry loops: widths up to 1 024 in one pass

// h1[b][c] = act(b0[c] + sum over the row's entries of coef_e * W0T[item_e][c]), entries in batch order.  The entries'
// (item, coef) are staged in LDS a tile at a time, so the loop over them carries no dependent global load.
__global__ __launch_bounds__(kBlock) void k_vae_enc0(const int64_t *__restrict__ row_off, const int32_t *__restrict__ row_len,
                                                     const int32_t *__restrict__ ent_item, const float *__restrict__ ent_coef,
                                                     const float *__restrict__ W0T, const float *__restrict__ b0, int d1,
                                                     int act, float *__restrict__ out) {
    __shared__ int32_t s_item[kBlock];
    __shared__ float s_coef[kBlock];
    const int64_t b = blockIdx.x;
    const int64_t off = row_off[b];
    const int len = row_len[b];
    for (int c0 = 0; c0 < d1; c0 += kBlock * kVaeCols) {
        float acc[kVaeCols];
#pragma unroll
        for (int q = 0; q < kVaeCols; ++q) acc[q] = 0.f;
        for (int e0 = 0; e0 < len; e0 += kBlock) {
            const int n = (len - e0 < kBlock) ? len - e0 : kBlock;
            __syncthreads();
            if ((int)threadIdx.x < n) {
                s_item[threadIdx.x] = ent_item[off + e0 + threadIdx.x];
                s_coef[threadIdx.x] = ent_coef[off + e0 + threadIdx.x];
            }
            __syncthreads();
            for (int e = 0; e < n; ++e) {
                const float cf = s_coef[e];
                if (cf == 0.f) continue;
                const float *w = W0T + (int64_t)s_item[e] * d1;
#pragma unroll
                for (int q = 0; q < kVaeCols; ++q) {
                    const int c = c0 + q * kBlock + threadIdx.x;
                    if (c < d1) acc[q] = fmaf(cf, w[c], acc[q]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < kVaeCols; ++q) {
            const int c = c0 + q * kBlock + threadIdx.x;
            if (c < d1) {
                const float pre = acc[q] + b0[c];
                out[b * d1 + c] = act ? tanhf(pre) : pre;
            }
        }
    }
}

// The float4 forms of the two entry loops (width a multiple of 4): wave w of the workgroup takes the staged entries
// w, w + 4, ... and every lane 4 columns per 256, so a wave reads whole rows with 16-byte loads and the four waves keep
// four rows in flight; the four wave sums are added in wave order at the end.  Fixed order: the same bits every run.
constexpr int kVaeV4Cols = 4 * kWave * 4;       // columns per pass: 4 float4 per lane
__device__ __forceinline__ void vae_rows_acc_v4(const float *__restrict__ M, int d, int c0, const int32_t *s_row,
                                                const float *s_coef, int n, float4 (&acc)[4]) {
    const int lane = threadIdx.x % kWave, w = threadIdx.x / kWave;
    for (int j = w; j < n; j += kBlock / kWave) {
        const float cf = s_coef[j];
        if (cf == 0.f) continue;
        const float *r = M + (int64_t)s_row[j] * d;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = c0 + (q * kWave + lane) * 4;
            if (c < d) {
                const float4 x = *reinterpret_cast<const float4 *>(r + c);
                acc[q].x = fmaf(cf, x.x, acc[q].x);
                acc[q].y = fmaf(cf, x.y, acc[q].y);
                acc[q].z = fmaf(cf, x.z, acc[q].z);
                acc[q].w = fmaf(cf, x.w, acc[q].w);
            }
        }
    }
}
// the four waves' sums of slot t (columns c0 + 4t .. c0 + 4t + 3), added in wave order
__device__ __forceinline__ float4 vae_wave_sum_v4(const float4 (&acc)[4], float4 (*red)[kBlock]) {
    const int lane = threadIdx.x % kWave, w = threadIdx.x / kWave;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) red[w][q * kWave + lane] = acc[q];
    __syncthreads();
    const int t = threadIdx.x;
    float4 v = red[0][t];
    for (int k = 1; k < kBlock / kWave; ++k) {
        v.x += red[k][t].x;
        v.y += red[k][t].y;
        v.z += red[k][t].z;
        v.w += red[k][t].w;
    }
    return v;
}

__global__ __launch_bounds__(kBlock) void k_vae_enc0_v4(const int64_t *__restrict__ row_off, const int32_t *__restrict__ row_len,
                                                        const int32_t *__restrict__ ent_item, const float *__restrict__ ent_coef,
                                                        const float *__restrict__ W0T, const float *__restrict__ b0, int d1,
                                                        int act, float *__restrict__ out) {
    __shared__ int32_t s_item[kBlock];
    __shared__ float s_coef[kBlock];
    __shared__ float4 red[kBlock / kWave][kBlock];
    const int64_t b = blockIdx.x;
    const int64_t off = row_off[b];
    const int len = row_len[b];
    for (int c0 = 0; c0 < d1; c0 += kVaeV4Cols) {
        float4 acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int e0 = 0; e0 < len; e0 += kBlock) {
            const int n = (len - e0 < kBlock) ? len - e0 : kBlock;
            __syncthreads();
            if ((int)threadIdx.x < n) {
                s_item[threadIdx.x] = ent_item[off + e0 + threadIdx.x];
                s_coef[threadIdx.x] = ent_coef[off + e0 + threadIdx.x];
            }
            __syncthreads();
            vae_rows_acc_v4(W0T, d1, c0, s_item, s_coef, n, acc);
        }
        const float4 v = vae_wave_sum_v4(acc, red);
        const int c = c0 + 4 * (int)threadIdx.x;
        if (c < d1) {
            const float pre[4] = {v.x + b0[c], v.y + b0[c + 1], v.z + b0[c + 2], v.w + b0[c + 3]};
            for (int k = 0; k < 4; ++k) out[b * d1 + c + k] = act ? tanhf(pre[k]) : pre[k];
        }
    }
}

// out[m][n] = act(bias[n] + sum_z ws[z][m][n]) (slices in order; nslices == 0: out itself holds the product)
__global__ __launch_bounds__(kBlock) void k_vae_reduce(const float *__restrict__ ws, int nslices, int64_t M, int N,
                                                       const float *__restrict__ bias, int act, float *__restrict__ out,
                                                       int64_t ldo) {
    const int64_t len = M * N;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < len; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = e / N;
        const int n = (int)(e % N);
        float v;
        if (nslices) {
            v = ws[e];
            for (int z = 1; z < nslices; ++z) v += ws[(int64_t)z * len + e];
        } else {
            v = out[m * ldo + n];
        }
        if (bias) v += bias[n];
        if (act) v = tanhf(v);
        out[m * ldo + n] = v;
    }
}

// z = mu + eps * exp(logvar / 2) (train) or mu; per row the KL sum of 1 + logvar - mu^2 - exp(logvar) (fp64, column order)
__global__ __launch_bounds__(kBlock) void k_vae_reparam(const float *__restrict__ h, int64_t B, int lat, const float *__restrict__ eps_in,
                                                        int train, uint64_t seed, float *__restrict__ eps, float *__restrict__ z,
                                                        double *__restrict__ kl) {
    const int lh = lat / 2, lo = (lat + 1) / 2;
    for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < B; b += (int64_t)gridDim.x * blockDim.x) {
        double s = 0.0;
        for (int j = 0; j < lh; ++j) {
            const float mu = h[b * lat + j], lv = h[b * lat + lo + j];
            if (train) {
                const float ep = eps_in ? eps_in[b * lh + j] : vae_normal(seed, (uint64_t)(b * lh + j));
                eps[b * lh + j] = ep;
                const float sd = expf(0.5f * lv);
                z[b * lh + j] = ep * sd + mu;
            } else {
                z[b * lh + j] = mu;
            }
            s += (double)(1.f + lv - mu * mu - expf(lv));
        }
        if (kl) kl[b] = s;
    }
}

// per row b: lse over z = Zraw + bias (online max / sum-exp, fixed tree), CE_b, then Z <- dZ = (softmax * s_b - R_b) / B
__global__ __launch_bounds__(kBlock) void k_vae_softmax(float *__restrict__ Z, const float *__restrict__ bias, int64_t I,
                                                        const int64_t *__restrict__ row_off, const int32_t *__restrict__ row_len,
                                                        const int32_t *__restrict__ ent_item, const float *__restrict__ ent_val,
                                                        const double *__restrict__ rsum, int64_t B, double *__restrict__ ce) {
    __shared__ float smm[kBlock], sms[kBlock];
    __shared__ double smd[kBlock];
    const int64_t b = blockIdx.x;
    float *zr = Z + b * I;
    float m = -INFINITY, s = 0.f;
    for (int64_t i = threadIdx.x; i < I; i += blockDim.x) {
        const float v = zr[i] + bias[i];
        if (v > m) {
            s = s * expf(m - v) + 1.f;
            m = v;
        } else {
            s += expf(v - m);
        }
    }
    smm[threadIdx.x] = m;
    sms[threadIdx.x] = s;
    __syncthreads();
    for (int st = kBlock / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            const float m1 = smm[threadIdx.x], m2 = smm[threadIdx.x + st];
            const float s1 = sms[threadIdx.x], s2 = sms[threadIdx.x + st];
            const float mm = fmaxf(m1, m2);
            float ss;
            if (m1 == -INFINITY) ss = s2;
            else if (m2 == -INFINITY) ss = s1;
            else ss = s1 * expf(m1 - mm) + s2 * expf(m2 - mm);
            smm[threadIdx.x] = mm;
            sms[threadIdx.x] = ss;
        }
        __syncthreads();
    }
    const float lse = smm[0] + logf(sms[0]);
    const int64_t off = row_off[b];
    const int len = row_len[b];
    double rz = 0.0;
    for (int e = threadIdx.x; e < len; e += blockDim.x) {
        const int64_t it = ent_item[off + e];
        rz += (double)ent_val[off + e] * (double)(zr[it] + bias[it]);
    }
    const double srz = vae_block_sum(rz, smd);
    const double sb = rsum[b];
    if (threadIdx.x == 0) ce[b] = sb * (double)lse - srz;
    const float sbf = (float)sb, inv_b = 1.f / (float)B;
    __syncthreads();
    for (int64_t i = threadIdx.x; i < I; i += blockDim.x) zr[i] = expf(zr[i] + bias[i] - lse) * sbf * inv_b;
    __syncthreads();
    for (int e = threadIdx.x; e < len; e += blockDim.x) {
        const int64_t it = ent_item[off + e];
        zr[it] -= ent_val[off + e] * inv_b;
    }
}

// loss = mean CE + anneal * (-0.5 * mean KL): every thread sums a contiguous run of rows in order, the runs are added
// in a fixed tree (fp64)
__global__ __launch_bounds__(kBlock) void k_vae_loss(const double *__restrict__ ce, const double *__restrict__ kl,
                                                     const int32_t *__restrict__ row_bad, int64_t B, float anneal,
                                                     double *__restrict__ stats) {
    __shared__ double sm[kBlock];
    const int64_t per = (B + kBlock - 1) / kBlock, r0 = threadIdx.x * per, r1 = (r0 + per < B) ? r0 + per : B;
    double c = 0.0, k = 0.0, bad = 0.0;
    for (int64_t b = r0; b < r1; ++b) {
        c += ce[b];
        k += kl[b];
        bad += row_bad[b];
    }
    c = vae_block_sum(c, sm);
    k = vae_block_sum(k, sm);
    bad = vae_block_sum(bad, sm);
    if (threadIdx.x != 0) return;
    if (bad > 0.0) stats[DAISY_VAE_ST_BAD_ROWS] += bad;
    c /= (double)B;
    k = -0.5 * (k / (double)B);
    const double loss = c + (double)anneal * k;
    stats[DAISY_VAE_ST_CE] = c;
    stats[DAISY_VAE_ST_KL] = k;
    stats[DAISY_VAE_ST_LOSS] = loss;
    stats[DAISY_VAE_ST_LOSS_SUM] += loss;
    if (!(fabs(loss) <= 1.7976931348623157e308)) stats[DAISY_VAE_ST_NONFINITE] += 1.0;
}

// column sums in two fixed-order passes: part[k][n] = sum of rows [k*rows, (k+1)*rows) in order (blockIdx.y = k), then
// out[n] += the chunks' sums in chunk order
__global__ __launch_bounds__(kBlock) void k_vae_colsum_part(const float *__restrict__ X, int64_t M, int64_t N, int64_t rows,
                                                            float *__restrict__ part) {
    const int64_t m0 = blockIdx.y * rows, m1 = (m0 + rows < M) ? m0 + rows : M;
    for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int64_t m = m0; m < m1; ++m) s += X[m * N + n];
        part[blockIdx.y * N + n] = s;
    }
}
__global__ __launch_bounds__(kBlock) void k_vae_colsum_fin(const float *__restrict__ part, int nchunks, int64_t N,
                                                           float *__restrict__ out) {
    for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int k = 0; k < nchunks; ++k) s += part[k * N + n];
        out[n] += s;
    }
}

// G *= 1 - Y^2 (tanh')
__global__ __launch_bounds__(kBlock) void k_vae_tanh_bwd(float *__restrict__ G, const float *__restrict__ Y, int64_t n) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
        G[e] *= 1.f - Y[e] * Y[e];
}

// dz [B][lh] -> d(encoder output) [B][lat]: d mu = dz + anneal * mu / B, d logvar = dz * eps * std / 2 - anneal / (2B) *
// (1 - exp(logvar)); the middle column of an odd lat gets 0
__global__ __launch_bounds__(kBlock) void k_vae_reparam_bwd(const float *__restrict__ dz, const float *__restrict__ h,
                                                            const float *__restrict__ eps, int64_t B, int lat, int train,
                                                            float anneal, float *__restrict__ dh) {
    const int lh = lat / 2, lo = (lat + 1) / 2;
    const float kmu = anneal / (float)B, klv = -0.5f * anneal / (float)B;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < B * lat; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = e / lat;
        const int c = (int)(e % lat);
        float g = 0.f;
        if (c < lh) {
            g = dz[b * lh + c] + kmu * h[e];
        } else if (c >= lo) {
            const int j = c - lo;
            const float lv = h[e];
            const float ex = expf(lv);
            g = klv * (1.f - ex);
            if (train) g += 0.5f * dz[b * lh + j] * eps[b * lh + j] * expf(0.5f * lv);
        }
        dh[e] = g;
    }
}

// dW0T[item][c] += sum over the kept entries of the item (batch order: the sort is stable) of coef_e * dA[row_e][c].  The
// head of every run of equal items walks the run a tile of 256 sorted positions at a time: the tile's (coef, row) pairs
// are staged in LDS by all threads at once (the run's end is where the tile's matching prefix stops), then every
// thread adds the tile's rows into its columns - no dependent global load per entry, whatever the item's popularity.
__global__ __launch_bounds__(kBlock) void k_vae_w0grad(const int32_t *__restrict__ key, const int32_t *__restrict__ idx, int64_t E,
                                                       int64_t I, const int32_t *__restrict__ ent_row, const float *__restrict__ ent_coef,
                                                       const float *__restrict__ dA, int d1, float *__restrict__ gW0T) {
    __shared__ int32_t s_row[kBlock];
    __shared__ float s_coef[kBlock];
    for (int64_t p = blockIdx.x; p < E; p += gridDim.x) {
        const int32_t it = key[p];
        if (it < 0 || (int64_t)it >= I || (p > 0 && key[p - 1] == it)) continue;
        for (int c0 = 0; c0 < d1; c0 += kBlock * kVaeCols) {
            float acc[kVaeCols];
#pragma unroll
            for (int q = 0; q < kVaeCols; ++q) acc[q] = 0.f;
            for (int64_t q0 = p;; q0 += kBlock) {
                const int64_t qq = q0 + threadIdx.x;
                const bool m = qq < E && key[qq] == it;          // (sorted: the matches are a prefix of the tile)
                if (m) {
                    const int32_t e = idx[qq];
                    s_coef[threadIdx.x] = ent_coef[e];
                    s_row[threadIdx.x] = ent_row[e];
                }
                const int n = __syncthreads_count(m);
                for (int j = 0; j < n; ++j) {
                    const float cf = s_coef[j];
                    if (cf == 0.f) continue;
                    const float *g = dA + (int64_t)s_row[j] * d1;
#pragma unroll
                    for (int q = 0; q < kVaeCols; ++q) {
                        const int c = c0 + q * kBlock + threadIdx.x;
                        if (c < d1) acc[q] = fmaf(cf, g[c], acc[q]);
                    }
                }
                __syncthreads();
                if (n < kBlock) break;
            }
#pragma unroll
            for (int q = 0; q < kVaeCols; ++q) {
                const int c = c0 + q * kBlock + threadIdx.x;
                if (c < d1) gW0T[(int64_t)it * d1 + c] += acc[q];
            }
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_vae_w0grad_v4(const int32_t *__restrict__ key, const int32_t *__restrict__ idx, int64_t E,
                                                          int64_t I, const int32_t *__restrict__ ent_row,
                                                          const float *__restrict__ ent_coef, const float *__restrict__ dA, int d1,
                                                          float *__restrict__ gW0T) {
    __shared__ int32_t s_row[kBlock];
    __shared__ float s_coef[kBlock];
    __shared__ float4 red[kBlock / kWave][kBlock];
    for (int64_t p = blockIdx.x; p < E; p += gridDim.x) {
        const int32_t it = key[p];
        if (it < 0 || (int64_t)it >= I || (p > 0 && key[p - 1] == it)) continue;
        for (int c0 = 0; c0 < d1; c0 += kVaeV4Cols) {
            float4 acc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int64_t q0 = p;; q0 += kBlock) {
                const int64_t qq = q0 + threadIdx.x;
                const bool m = qq < E && key[qq] == it;          // (sorted: the matches are a prefix of the tile)
                if (m) {
                    const int32_t e = idx[qq];
                    s_coef[threadIdx.x] = ent_coef[e];
                    s_row[threadIdx.x] = ent_row[e];
                }
                const int n = __syncthreads_count(m);
                vae_rows_acc_v4(dA, d1, c0, s_row, s_coef, n, acc);
                __syncthreads();
                if (n < kBlock) break;
            }
            const float4 v = vae_wave_sum_v4(acc, red);
            const int c = c0 + 4 * (int)threadIdx.x;
            if (c < d1) {
                float *gr = gW0T + (int64_t)it * d1 + c;
                gr[0] += v.x;
                gr[1] += v.y;
                gr[2] += v.z;
                gr[3] += v.w;
            }
        }
    }
}

// rank: out[b][c] = bias[item] + <H[b], Wout[item]> for item = items[b][c], one wave per pair (lanes over the width)
__global__ __launch_bounds__(kBlock) void k_vae_gather_scores(const float *__restrict__ H, const float *__restrict__ Wout,
                                                              const float *__restrict__ bias, int w, const int64_t *__restrict__ items,
                                                              int64_t B, int64_t C, int64_t I, float *__restrict__ out) {
    const int lane = threadIdx.x % kWave;
    const int64_t waves = (int64_t)gridDim.x * (kBlock / kWave);
    for (int64_t p = blockIdx.x * (int64_t)(kBlock / kWave) + threadIdx.x / kWave; p < B * C; p += waves) {
        const int64_t b = p / C, it = items[p];
        const bool ok = it >= 0 && it < I;
        float s = 0.f;
        if (ok)
            for (int c = lane; c < w; c += kWave) s = fmaf(H[b * w + c], Wout[it * w + c], s);
        for (int o = kWave / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, kWave);
        if (lane == 0) out[p] = ok ? s + bias[it] : NAN;
    }
}

}  // namespace daisy

using namespace daisy;

struct daisy_vae_ctx {
    int64_t max_batch, max_entries, item_num;
    int n_hidden, lat;
    int hidden[DAISY_VAE_MAX_HIDDEN];
    int enc[DAISY_VAE_MAX_HIDDEN + 2];          // encoder widths: I, hidden..., lat
    int dec[DAISY_VAE_MAX_HIDDEN + 2];          // decoder widths: lat/2, reversed hidden..., I
    int64_t w_off[2][DAISY_VAE_MAX_HIDDEN + 1]; // flat offsets of the weights / biases of every layer (0 encoder, 1 decoder)
    int64_t b_off[2][DAISY_VAE_MAX_HIDDEN + 1];
    int64_t n_params;
    int maxw;                                   // widest hidden / latent layer
    DeviceArena arena;
    int32_t *ent_item, *ent_row, *ent_idx, *kout, *vout, *row_len, *row_bad;
    float *ent_coef, *ent_val;
    int64_t *row_off;
    double *rsum, *ce, *kl;
    float *act[2][DAISY_VAE_MAX_HIDDEN + 2];    // activations: [0][l] encoder output of layer l-1 (l >= 1), [1][k] decoder
    float *eps, *logits, *G1, *G2, *ws;
    size_t ws_floats;
    void *sort_tmp;
    size_t sort_bytes;
};

namespace {

// the product of one Linear layer (or of its gradients): split-k to about kVaeTargetTiles workgroups, the slices summed
// in order by k_vae_reduce together with the bias and the activation; a product that needs neither goes straight to C
int vae_gemm(daisy_vae_ctx *c, const float *A, int64_t sam, int64_t sak, const float *Bm, int64_t sbn, int64_t sbk, float *C,
             int64_t ldc, int64_t M, int N, int64_t K, const float *bias, int act, hipStream_t s) {
    const int64_t bn = N > 64 ? 128 : 64;
    const int64_t tiles = ((M + 127) / 128) * ((N + bn - 1) / bn);
    int64_t splits = 1;
    if (tiles < kVaeTargetTiles / 2) {
        splits = (kVaeTargetTiles + tiles - 1) / tiles;
        const int64_t kmax = K / 64 > 1 ? K / 64 : 1;                // at least 64 k per slice
        if (splits > kmax) splits = kmax;
        if (splits > 64) splits = 64;
        while (splits > 1 && (size_t)(splits * M * N) > c->ws_floats) --splits;
    }
    int64_t k_chunk = K;
    if (splits > 1) {
        k_chunk = ((K + splits - 1) / splits + 15) / 16 * 16;
        splits = (K + k_chunk - 1) / k_chunk;
    }
    if (splits <= 1) {
        gemm_f32(A, sam, sak, Bm, sbn, sbk, C, ldc, M, N, K, K, 0, s);
        DAISY_LAUNCH_CHECK();
        if (bias || act) {
            hipLaunchKernelGGL(k_vae_reduce, dim3(grid_for(M * N, kBlock)), dim3(kBlock), 0, s, (const float *)nullptr, 0, M, N,
                               bias, act, C, ldc);
            DAISY_LAUNCH_CHECK();
        }
        return DAISY_OK;
    }
    gemm_f32(A, sam, sak, Bm, sbn, sbk, c->ws, N, M, N, K, k_chunk, M * N, s);
    DAISY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_vae_reduce, dim3(grid_for(M * N, kBlock)), dim3(kBlock), 0, s, c->ws, (int)splits, M, N, bias, act, C, ldc);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

const float *P(const float *W, int64_t off) { return W + off; }

// out[n] += sum_m X[m][n] over M rows, in chunks of about sqrt(M) rows (at least 16): both passes walk about sqrt(M)
// values per thread (the chunk sums live in the split-k workspace)
int vae_colsum(daisy_vae_ctx *c, const float *X, int64_t M, int64_t N, float *out, hipStream_t s) {
    int64_t rows0 = 16;
    while (rows0 * rows0 < M) ++rows0;
    int64_t nchunks = (M + rows0 - 1) / rows0;
    const int64_t cap = (int64_t)(c->ws_floats / (size_t)N);
    if (nchunks > cap) nchunks = cap > 1 ? cap : 1;
    const int64_t rows = (M + nchunks - 1) / nchunks;
    nchunks = (M + rows - 1) / rows;
    hipLaunchKernelGGL(k_vae_colsum_part, dim3(grid_for(N, kBlock, 512), (unsigned)nchunks), dim3(kBlock), 0, s, X, M, N, rows, c->ws);
    DAISY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_vae_colsum_fin, dim3(grid_for(N, kBlock)), dim3(kBlock), 0, s, c->ws, (int)nchunks, N, out);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

// the forward pass of B users up to the last decoder layer's input (c->act[1][n_hidden]); z in c->act[1][0], the rows' KL
// sums in c->kl
int vae_forward(daisy_vae_ctx *c, const float *W, const VaeBatch &vb, const float *eps_in, hipStream_t s) {
    const int64_t B = vb.B;
    const int n = c->n_hidden, lat = c->lat;
    hipLaunchKernelGGL(k_vae_offsets, dim3(1), dim3(kBlock), 0, s, vb, c->row_off);
    DAISY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_vae_prep, dim3((unsigned)B), dim3(kBlock), 0, s, vb, c->ent_item, c->ent_row, c->ent_idx, c->ent_coef,
                       c->ent_val, (const int64_t *)c->row_off, c->row_len, c->rsum, c->row_bad);
    DAISY_LAUNCH_CHECK();
    const bool v4 = c->enc[1] % 4 == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0;    // (W0T is the buffer's first tensor)
    hipLaunchKernelGGL(v4 ? k_vae_enc0_v4 : k_vae_enc0, dim3((unsigned)B), dim3(kBlock), 0, s, c->row_off, c->row_len, c->ent_item,
                       c->ent_coef, P(W, c->w_off[0][0]), P(W, c->b_off[0][0]), c->enc[1], n > 0 ? 1 : 0, c->act[0][1]);
    DAISY_LAUNCH_CHECK();
    for (int l = 1; l <= n; ++l) {
        const int din = c->enc[l], dout = c->enc[l + 1];
        if (int rc = vae_gemm(c, c->act[0][l], din, 1, P(W, c->w_off[0][l]), din, 1, c->act[0][l + 1], dout, B, dout, din,
                              P(W, c->b_off[0][l]), l < n ? 1 : 0, s))
            return rc;
    }
    hipLaunchKernelGGL(k_vae_reparam, dim3(grid_for(B, kBlock)), dim3(kBlock), 0, s, c->act[0][n + 1], B, lat, eps_in, vb.train,
                       vb.seed, c->eps, c->act[1][0], c->kl);
    DAISY_LAUNCH_CHECK();
    for (int k = 0; k < n; ++k) {
        const int din = c->dec[k], dout = c->dec[k + 1];
        if (int rc = vae_gemm(c, c->act[1][k], din, 1, P(W, c->w_off[1][k]), din, 1, c->act[1][k + 1], dout, B, dout, din,
                              P(W, c->b_off[1][k]), 1, s))
            return rc;
    }
    return DAISY_OK;
}

int vae_check_batch(const daisy_vae_ctx *c, const int64_t *row_ptr, const int32_t *col, const float *val, int64_t user_num,
                    const int64_t *users, int64_t B, int64_t n_entries, float dropout_p, const char *what) {
    DAISY_CHECK_ARG(row_ptr && users && (n_entries == 0 || (col && val)), "%s: null CSR / users pointer", what);
    DAISY_CHECK_ARG(user_num >= 1, "%s: user_num=%lld", what, (long long)user_num);
    DAISY_CHECK_ARG(B >= 1 && B <= c->max_batch, "%s: B=%lld (1 .. %lld)", what, (long long)B, (long long)c->max_batch);
    DAISY_CHECK_ARG(n_entries >= 0 && n_entries <= c->max_entries, "%s: n_entries=%lld (0 .. %lld)", what, (long long)n_entries,
                    (long long)c->max_entries);
    DAISY_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "%s: dropout=%g (0 <= p < 1)", what, (double)dropout_p);
    return DAISY_OK;
}

VaeBatch vae_batch(const daisy_vae_ctx *c, const int64_t *row_ptr, const int32_t *col, const float *val, int64_t user_num,
                   const int64_t *users, int64_t B, int64_t n_entries, const uint8_t *keep, int train, float dropout_p,
                   uint64_t seed) {
    VaeBatch vb{};
    vb.row_ptr = row_ptr;
    vb.col = col;
    vb.val = val;
    vb.user_num = user_num;
    vb.users = users;
    vb.B = B;
    vb.n_entries = n_entries;
    vb.item_num = c->item_num;
    vb.keep = keep;
    vb.thresh = train ? keep_threshold(dropout_p) : 0u;
    vb.scale = (train && dropout_p > 0.f) ? 1.f / (1.f - dropout_p) : 1.f;
    if (keep && train && dropout_p > 0.f && vb.thresh == 0u) vb.thresh = 1u;     // (caller's bits: only "dropout on" matters)
    vb.train = train ? 1 : 0;
    vb.seed = seed;
    return vb;
}

int vae_step(daisy_vae_ctx *c, const float *W, float *g, const VaeBatch &vb, const float *eps_in, float anneal, double *stats,
             hipStream_t s) {
    const int64_t B = vb.B, I = c->item_num, E = vb.n_entries;
    const int n = c->n_hidden, lat = c->lat;
    if (int rc = vae_forward(c, W, vb, eps_in, s)) return rc;
    // logits [B][I] without the bias (k_vae_softmax adds it)
    const int wl = c->dec[n];
    const float *Wout = P(W, c->w_off[1][n]), *bout = P(W, c->b_off[1][n]);
    if (int rc = vae_gemm(c, c->act[1][n], wl, 1, Wout, wl, 1, c->logits, I, B, (int)I, wl, nullptr, 0, s)) return rc;
    hipLaunchKernelGGL(k_vae_softmax, dim3((unsigned)B), dim3(kBlock), 0, s, c->logits, bout, I, c->row_off, c->row_len, c->ent_item,
                       c->ent_val, c->rsum, B, c->ce);
    DAISY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_vae_loss, dim3(1), dim3(kBlock), 0, s, c->ce, c->kl, c->row_bad, B, anneal, stats);
    DAISY_LAUNCH_CHECK();
    // ---- backward.  dZ in c->logits
    const float *dZ = c->logits;
    if (int rc = vae_colsum(c, dZ, B, I, g + c->b_off[1][n], s)) return rc;
    // dW_out [I][wl] = dZ^T H: A(m = item, k = row) = dZ[row * I + item], B(n = col, k = row) = H[row * wl + col]
    if (int rc = vae_gemm(c, dZ, 1, I, c->act[1][n], 1, wl, g + c->w_off[1][n], wl, I, wl, B, nullptr, 0, s)) return rc;
    // dH [B][wl] = dZ W_out: A(m = row, k = item) = dZ[row * I + item], B(n = col, k = item) = Wout[item * wl + col]
    float *G = c->G1, *G2 = c->G2;
    if (int rc = vae_gemm(c, dZ, I, 1, Wout, 1, wl, G, wl, B, wl, I, nullptr, 0, s)) return rc;
    for (int k = n; k >= 1; --k) {
        // G = d D_k [B][dec[k]]; D_k = tanh(D_{k-1} V_{k-1}^T + c_{k-1})
        const int dout = c->dec[k], din = c->dec[k - 1];
        hipLaunchKernelGGL(k_vae_tanh_bwd, dim3(grid_for(B * dout, kBlock)), dim3(kBlock), 0, s, G, c->act[1][k], B * dout);
        DAISY_LAUNCH_CHECK();
        if (int rc = vae_colsum(c, G, B, dout, g + c->b_off[1][k - 1], s)) return rc;
        if (int rc = vae_gemm(c, G, 1, dout, c->act[1][k - 1], 1, din, g + c->w_off[1][k - 1], din, dout, din, B, nullptr, 0, s))
            return rc;
        const float *V = P(W, c->w_off[1][k - 1]);         // [dout][din]: B(n = col, k = j) = V[j * din + col]
        if (int rc = vae_gemm(c, G, dout, 1, V, 1, din, G2, din, B, din, dout, nullptr, 0, s)) return rc;
        float *t = G;
        G = G2;
        G2 = t;
    }
    // G = dz [B][lh] -> d(encoder output) [B][lat] in G2
    hipLaunchKernelGGL(k_vae_reparam_bwd, dim3(grid_for(B * lat, kBlock)), dim3(kBlock), 0, s, G, c->act[0][n + 1], c->eps, B, lat,
                       vb.train, anneal, G2);
    DAISY_LAUNCH_CHECK();
    {
        float *t = G;
        G = G2;
        G2 = t;
    }
    for (int l = n; l >= 1; --l) {
        // G = d(pre-activation of encoder layer l) [B][enc[l+1]]; its input E_l = act[0][l] [B][enc[l]] (post-tanh)
        const int dout = c->enc[l + 1], din = c->enc[l];
        if (int rc = vae_colsum(c, G, B, dout, g + c->b_off[0][l], s)) return rc;
        if (int rc = vae_gemm(c, G, 1, dout, c->act[0][l], 1, din, g + c->w_off[0][l], din, dout, din, B, nullptr, 0, s)) return rc;
        const float *Wl = P(W, c->w_off[0][l]);
        if (int rc = vae_gemm(c, G, dout, 1, Wl, 1, din, G2, din, B, din, dout, nullptr, 0, s)) return rc;
        hipLaunchKernelGGL(k_vae_tanh_bwd, dim3(grid_for(B * din, kBlock)), dim3(kBlock), 0, s, G2, c->act[0][l], B * din);
        DAISY_LAUNCH_CHECK();
        float *t = G;
        G = G2;
        G2 = t;
    }
    // G = d(pre-activation of the sparse layer) [B][enc[1]]
    const int d1 = c->enc[1];
    if (int rc = vae_colsum(c, G, B, d1, g + c->b_off[0][0], s)) return rc;
    if (E > 0) {
        const int bits = bits_for(I + 1);                                // ids 0 .. I (I: the padding sentinel)
        if (int rc = sort_pairs_i32(c->sort_tmp, c->sort_bytes, c->ent_item, c->kout, c->ent_idx, c->vout, E, bits, s)) return rc;
        const bool v4 = d1 % 4 == 0 && (reinterpret_cast<uintptr_t>(g) & 15) == 0;      // (G: an arena slot, 256-byte aligned)
        hipLaunchKernelGGL(v4 ? k_vae_w0grad_v4 : k_vae_w0grad, dim3(grid_for(E, 1, kMaxGridSparse)), dim3(kBlock), 0, s, c->kout,
                           c->vout, E, I, c->ent_row, c->ent_coef, G, d1, g + c->w_off[0][0]);
        DAISY_LAUNCH_CHECK();
    }
    return DAISY_OK;
}

}  // namespace

extern "C" {

int daisy_vae_ctx_create(daisy_vae_ctx **out, int64_t max_batch, int64_t max_entries, int64_t item_num, int32_t n_hidden,
                         const int32_t *hidden, int32_t latent_dim) {
    DAISY_CHECK_ARG(out, "vae_ctx_create: out is NULL");
    *out = nullptr;
    DAISY_CHECK_ARG(max_batch >= 1 && max_batch <= (1ll << 20), "vae_ctx_create: max_batch=%lld (1 .. 2^20)", (long long)max_batch);
    DAISY_CHECK_ARG(max_entries >= 0 && max_entries < (1ll << 31), "vae_ctx_create: max_entries=%lld (0 .. 2^31 - 1)",
                    (long long)max_entries);
    // (item_num < 2^24: the GEMM epilogue addresses a 128-row tile of the [B][item_num] logits with 32-bit offsets)
    DAISY_CHECK_ARG(item_num >= 1 && item_num < (1ll << 24), "vae_ctx_create: item_num=%lld (1 .. 2^24 - 1)", (long long)item_num);
    DAISY_CHECK_ARG(n_hidden >= 0 && n_hidden <= DAISY_VAE_MAX_HIDDEN, "vae_ctx_create: n_hidden=%d (0 .. %d)", n_hidden,
                    DAISY_VAE_MAX_HIDDEN);
    DAISY_CHECK_ARG(n_hidden == 0 || hidden, "vae_ctx_create: hidden is NULL");
    for (int l = 0; l < n_hidden; ++l)
        DAISY_CHECK_ARG(hidden[l] >= 1 && hidden[l] <= (1 << 16), "vae_ctx_create: hidden[%d]=%d (1 .. 65536)", l, hidden[l]);
    DAISY_CHECK_ARG(latent_dim >= 2 && latent_dim <= (1 << 16), "vae_ctx_create: latent_dim=%d (2 .. 65536)", latent_dim);
    DAISY_CHECK_ARG(max_batch * item_num < (1ll << 40), "vae_ctx_create: max_batch x item_num too large");
    daisy_vae_ctx *c = new daisy_vae_ctx();
    c->max_batch = max_batch;
    c->max_entries = max_entries;
    c->item_num = item_num;
    c->n_hidden = n_hidden;
    c->lat = latent_dim;
    const int n = n_hidden;
    c->enc[0] = (int)item_num;
    for (int l = 0; l < n; ++l) c->hidden[l] = c->enc[l + 1] = hidden[l];
    c->enc[n + 1] = latent_dim;
    c->dec[0] = latent_dim / 2;
    for (int k = 1; k <= n; ++k) c->dec[k] = hidden[n - k];
    c->dec[n + 1] = (int)item_num;
    int64_t off = 0;
    for (int l = 0; l <= n; ++l) {                  // encoder.{2l}.weight, .bias
        c->w_off[0][l] = off;
        off += (int64_t)c->enc[l] * c->enc[l + 1];
        c->b_off[0][l] = off;
        off += c->enc[l + 1];
    }
    for (int k = 0; k <= n; ++k) {                  // decoder.{2k}.weight, .bias
        c->w_off[1][k] = off;
        off += (int64_t)c->dec[k] * c->dec[k + 1];
        c->b_off[1][k] = off;
        off += c->dec[k + 1];
    }
    c->n_params = off;
    int maxw = latent_dim;
    for (int l = 0; l < n; ++l) maxw = hidden[l] > maxw ? hidden[l] : maxw;
    c->maxw = maxw;
    const int64_t Bm = max_batch, Em = max_entries > 0 ? max_entries : 1;
    c->ws_floats = (size_t)(kVaeTargetTiles + 64) * 128 * 128;      // split-k slices; column-sum chunks (>= one row of I)
    if (c->ws_floats < (size_t)item_num * 4) c->ws_floats = (size_t)item_num * 4;
    c->sort_bytes = sort_pairs_i32_temp_bytes_upto(Em);
    DeviceArena &a = c->arena;
    a.add(&c->ent_item, Em * 4); a.add(&c->ent_row, Em * 4); a.add(&c->ent_idx, Em * 4); a.add(&c->kout, Em * 4);
    a.add(&c->vout, Em * 4); a.add(&c->ent_coef, Em * 4); a.add(&c->ent_val, Em * 4);
    a.add(&c->row_len, Bm * 4); a.add(&c->row_bad, Bm * 4);
    a.add(&c->row_off, Bm * 8); a.add(&c->rsum, Bm * 8); a.add(&c->ce, Bm * 8); a.add(&c->kl, Bm * 8);
    for (int l = 1; l <= n + 1; ++l) a.add(&c->act[0][l], (size_t)Bm * c->enc[l] * 4);
    for (int k = 0; k <= n; ++k) a.add(&c->act[1][k], (size_t)Bm * c->dec[k] * 4);
    a.add(&c->eps, (size_t)Bm * c->dec[0] * 4); a.add(&c->logits, (size_t)Bm * item_num * 4);
    a.add(&c->G1, (size_t)Bm * maxw * 4); a.add(&c->G2, (size_t)Bm * maxw * 4);
    a.add(&c->ws, c->ws_floats * 4); a.add(&c->sort_tmp, c->sort_bytes);
    if (int rc = a.alloc("vae_ctx_create")) {
        delete c;
        return rc;
    }
    *out = c;
    return DAISY_OK;
}

int daisy_vae_ctx_destroy(daisy_vae_ctx *ctx) {
    if (!ctx) return DAISY_OK;
    ctx->arena.release();
    delete ctx;
    return DAISY_OK;
}

size_t daisy_vae_ctx_bytes(const daisy_vae_ctx *ctx) { return ctx ? ctx->arena.bytes() : 0; }

int64_t daisy_vae_param_count(const daisy_vae_ctx *ctx) { return ctx ? ctx->n_params : 0; }

int daisy_vae_step_grads(daisy_vae_ctx *ctx, const float *W, float *g, const int64_t *row_ptr, const int32_t *col,
                         const float *val, int64_t user_num, const int64_t *users, int64_t B, int64_t n_entries,
                         const uint8_t *keep, const float *eps, int32_t train, float dropout_p, float anneal, uint64_t seed,
                         double *stats, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && W && g && stats, "vae_step_grads: null argument");
    if (int rc = vae_check_batch(ctx, row_ptr, col, val, user_num, users, B, n_entries, dropout_p, "vae_step_grads")) return rc;
    DAISY_CHECK_ARG(anneal >= 0.f && anneal <= 1e30f, "vae_step_grads: anneal=%g", (double)anneal);
    const VaeBatch vb = vae_batch(ctx, row_ptr, col, val, user_num, users, B, n_entries, keep, train, dropout_p, seed);
    return vae_step(ctx, W, g, vb, train ? eps : nullptr, anneal, stats, as_stream(stream));
}

int daisy_vae_fit_epoch(daisy_vae_ctx *ctx, float *W, float *g, const int64_t *row_ptr, const int32_t *col, const float *val,
                        int64_t user_num, const int64_t *users, int64_t n, int64_t batch, const int64_t *entries,
                        float dropout_p, double anneal_cap, int64_t total_anneal_steps, int64_t update0, uint64_t seed_hi,
                        int64_t step0, int64_t opt_step0, int32_t optimizer, float lr, float *state0, float *state1,
                        double *stats, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && W && g && stats && entries && users && n > 0 && batch > 0 && step0 >= 0 && opt_step0 >= 0 && update0 >= 0,
                    "vae_fit_epoch: bad argument");
    if (int rc = dense_opt_check("vae_fit_epoch", optimizer, state0, state1)) return rc;
    DAISY_CHECK_ARG(anneal_cap >= 0.0 && anneal_cap <= 1e30, "vae_fit_epoch: anneal_cap=%g", anneal_cap);
    const int64_t nb = (n + batch - 1) / batch;
    for (int64_t k = 0; k < nb; ++k) {
        const int64_t B = (n - k * batch < batch) ? n - k * batch : batch;
        if (int rc = vae_check_batch(ctx, row_ptr, col, val, user_num, users + k * batch, B, entries[k], dropout_p, "vae_fit_epoch"))
            return rc;
    }
    hipStream_t s = as_stream(stream);
    const int64_t nf = ctx->n_params;
    int64_t t = opt_step0;
    for (int64_t k = 0; k < nb; ++k) {
        const int64_t B = (n - k * batch < batch) ? n - k * batch : batch;
        const int64_t update = update0 + k + 1;
        double an = anneal_cap;
        if (total_anneal_steps > 0) {
            const double r = 1.0 * (double)update / (double)total_anneal_steps;
            an = anneal_cap < r ? anneal_cap : r;
        }
        const VaeBatch vb = vae_batch(ctx, row_ptr, col, val, user_num, users + k * batch, B, entries[k], nullptr, 1, dropout_p,
                                      seed_hi | (uint64_t)(step0 + k + 1));
        if (int rc = vae_step(ctx, W, g, vb, nullptr, (float)an, stats, s)) return rc;
        ++t;
        if (int rc = dense_opt_step(optimizer, W, g, state0, state1, nf, lr, t, stream)) return rc;
    }
    return DAISY_OK;
}

int daisy_vae_scores(daisy_vae_ctx *ctx, const float *W, const int64_t *row_ptr, const int32_t *col, const float *val,
                     int64_t user_num, const int64_t *users, int64_t B, int64_t n_entries, const int64_t *items, int64_t C,
                     const uint8_t *keep, const float *eps, int32_t train, float dropout_p, uint64_t seed, float *out,
                     daisy_stream_t stream) {
    DAISY_CHECK_ARG(ctx && W && out, "vae_scores: null argument");
    if (int rc = vae_check_batch(ctx, row_ptr, col, val, user_num, users, B, n_entries, dropout_p, "vae_scores")) return rc;
    DAISY_CHECK_ARG(!items || C >= 1, "vae_scores: C=%lld with candidates", (long long)C);
    hipStream_t s = as_stream(stream);
    const VaeBatch vb = vae_batch(ctx, row_ptr, col, val, user_num, users, B, n_entries, keep, train, dropout_p, seed);
    if (int rc = vae_forward(ctx, W, vb, train ? eps : nullptr, s)) return rc;      // (user ids: checked by the caller)
    const int n = ctx->n_hidden, wl = ctx->dec[n];
    const int64_t I = ctx->item_num;
    const float *Wout = P(W, ctx->w_off[1][n]), *bout = P(W, ctx->b_off[1][n]);
    if (items) {
        hipLaunchKernelGGL(k_vae_gather_scores, dim3(grid_for(B * C, kBlock / kWave, 8192)), dim3(kBlock), 0, s, ctx->act[1][n], Wout,
                           bout, wl, items, B, C, I, out);
        DAISY_LAUNCH_CHECK();
        return DAISY_OK;
    }
    return vae_gemm(ctx, ctx->act[1][n], wl, 1, Wout, wl, 1, out, I, B, (int)I, wl, bout, 0, s);
}

}  // extern "C"
