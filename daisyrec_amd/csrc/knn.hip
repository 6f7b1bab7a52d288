// ItemKNN / UserKNN (daisy/model/KNNCFRecommender.py): the similarity of the columns of a data matrix D from
// its Gram matrix G = D^T D (daisy_slim_gram), the K largest weights of every column by a radix select, and the fp64 scores
// of a sparse row times a sparse column.  No floating-point atomics: the only atomics are integer counts in LDS, whose sum
// does not depend on their order, so every output is the same run after run.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "score_f64.h"
#include "topk_f64.h"

namespace daisy {
namespace {

constexpr int kKnnWaves = kBlock / kWave;
constexpr int kKnnRankLdsItems = 32768;            // a row of L, dense: 128 KB
constexpr uint32_t kKnnZeroKey = 0x80000000u;      // the key of +0.0 and of -0.0

inline bool knn_mode_ok(int32_t mode) { return mode >= DAISY_KNN_COSINE && mode <= DAISY_KNN_PLAIN; }
inline size_t knn_out_bytes(int64_t n, int64_t K) {
    return align_up((size_t)n * sizeof(int32_t)) + 2 * align_up((size_t)n * (size_t)K * sizeof(float)) +
           align_up((size_t)n * sizeof(float));
}

// ---- means and centring ----------------------------------------------------------------------------------------------
// One wave per row: lane l adds the entries beg + l, beg + l + 64, ... in that order, then the lanes meet in a xor tree.
__global__ __launch_bounds__(kBlock) void k_knn_row_means(const int64_t *__restrict__ row_ptr, const float *__restrict__ val,
                                                          int64_t n_rows, float *__restrict__ mean) {
    const int lane = threadIdx.x % kWave;
    const int64_t wave = blockIdx.x * (int64_t)kKnnWaves + threadIdx.x / kWave;
    for (int64_t r = wave; r < n_rows; r += (int64_t)gridDim.x * kKnnWaves) {
        const int64_t beg = row_ptr[r], end = row_ptr[r + 1];
        float s = 0.f;
        for (int64_t e = beg + lane; e < end; e += kWave) s += val[e];
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
        if (lane == 0) mean[r] = end > beg ? __fdiv_rn(s, (float)(end - beg)) : 0.f;
    }
}

__global__ __launch_bounds__(kBlock) void k_knn_center(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                       const float *val, int64_t n_rows, int64_t n_cols, int mode,
                                                       const float *__restrict__ mean, float *out) {
    for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const int64_t beg = row_ptr[r], end = row_ptr[r + 1];
        const float rm = mode == DAISY_KNN_CENTER_ROW ? mean[r] : 0.f;
        for (int64_t e = beg + threadIdx.x; e < end; e += kBlock) {
            float v = val[e];
            if (mode == DAISY_KNN_CENTER_ROW) {
                v -= rm;
            } else if (mode == DAISY_KNN_CENTER_COL) {
                const int32_t c = col[e];
                v -= (c >= 0 && c < n_cols) ? mean[c] : 0.f;
            } else if (mode == DAISY_KNN_CENTER_BINARY) {
                v = 1.f;
            }
            out[e] = v;
        }
    }
}

// ss[i] = G[i, i], square-rooted unless the similarity is one of the binary ones.  The root is taken in fp64 and rounded
// once more: correctly rounded in fp32 (53 >= 2 * 24 + 2 bits), which the fp32 intrinsics do not promise.
__global__ __launch_bounds__(kBlock) void k_knn_diag(const float *__restrict__ G, int64_t n, int take_sqrt,
                                                     float *__restrict__ ss) {
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const float d = G[i * n + i];
        ss[i] = take_sqrt ? (float)sqrt((double)d) : d;
    }
}

// ---- the weight of one pair ------------------------------------------------------------------------------------------
// KNNCFRecommender.py:313-337 in fp32, operation by operation: every sum, the reciprocal and the product are rounded on
// their own, so nothing from here on is contracted into a fused multiply-add (the scores' products are exact in fp64).
#pragma clang fp contract(off)
struct KnnWeight {
    int mode;
    float shrink, eps;
    float ssj;              // ss[j]; ASYMMETRIC: ss[j]^(2 alpha)
    float pow_other;        // ASYMMETRIC: 2 (1 - alpha)
};

__device__ __forceinline__ float knn_weight(const KnnWeight &p, float g, float ssi, bool self) {
    const float w = self ? 0.f : g;
    float den;
    switch (p.mode) {
    case DAISY_KNN_COSINE: den = p.ssj * ssi + p.shrink + p.eps; break;
    case DAISY_KNN_ASYMMETRIC: den = p.ssj * powf(ssi, p.pow_other) + p.shrink + p.eps; break;
    case DAISY_KNN_TANIMOTO: den = p.ssj + ssi - w + p.shrink + p.eps; break;
    case DAISY_KNN_DICE: den = p.ssj + ssi + p.shrink + p.eps; break;
    case DAISY_KNN_TVERSKY: den = w + (p.ssj - w) + (ssi - w) + p.shrink + p.eps; break;
    default: return p.shrink != 0.f ? __fdiv_rn(w, p.shrink) : w;
    }
    return w * __fdiv_rn(1.f, den);
}

// larger value <=> larger key; both zeros share one key; a value that is not a number sorts below everything
__device__ __forceinline__ uint32_t knn_key(float w) {
    if (w != w) return 0u;
    if (w == 0.f) return kKnnZeroKey;
    const uint32_t u = __float_as_uint(w);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ---- select ----------------------------------------------------------------------------------------------------------
// One workgroup per column at a time.  Four histogram passes (8 bits each, from the top) find the key of the keff-th
// largest weight and how many entries with exactly that key belong to the keff largest; one more pass in ascending row
// order hands out the slots.  The weights are recomputed by the same code on every pass: bit-identical, nothing staged, so
// the length of a row is not bounded by the LDS (a long row comes from L2 again).
__global__ __launch_bounds__(kBlock) void k_knn_select(const float *__restrict__ G, const float *__restrict__ ss, int64_t n,
                                                       int mode, float shrink, float alpha, int K,
                                                       int32_t *__restrict__ count, int32_t *__restrict__ rows,
                                                       float *__restrict__ vals) {
    __shared__ __attribute__((aligned(16))) int s_hist[4][256];
    __shared__ int s_cnt[2][kKnnWaves][2];
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int keff = (int64_t)K < n ? K : (int)n;

    for (int64_t j = blockIdx.x; j < n; j += gridDim.x) {
        const float *__restrict__ g = G + j * n;          // G is symmetric: column j is the contiguous row j
        KnnWeight p;
        p.mode = mode;
        p.shrink = shrink;
        p.eps = 1e-6f;
        p.ssj = ss[j];
        p.pow_other = 0.f;
        if (mode == DAISY_KNN_ASYMMETRIC) {
            p.ssj = powf(p.ssj, 2.f * alpha);
            p.pow_other = 2.f * (1.f - alpha);
        }
        for (int e = tid; e < 4 * 256; e += kBlock) (&s_hist[0][0])[e] = 0;
        __syncthreads();

        uint32_t prefix = 0u;
        int krem = keff;                                    // the rank wanted among the keys that match the prefix
#pragma unroll 1
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            const uint32_t hi_mask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
            int *hist = s_hist[pass];
            for (int64_t base = 0; base < n; base += kBlock) {
                const int64_t i = base + tid;
                bool in = false, zero = false;
                uint32_t key = 0u;
                if (i < n) {
                    key = knn_key(knn_weight(p, g[i], ss[i], i == j));
                    in = (key & hi_mask) == prefix;
                    zero = in && key == kKnnZeroKey;
                }
                // the zeros of a sparse column would all hit one counter: a wave counts its own with a ballot
                const unsigned long long zm = __ballot(zero);
                if (zm && lane == __ffsll((long long)zm) - 1) atomicAdd(&hist[(kKnnZeroKey >> shift) & 255], __popcll(zm));
                if (in && !zero) atomicAdd(&hist[(key >> shift) & 255], 1);
            }
            __syncthreads();
            // every wave finds the digit for itself: lane l owns the digits 4 l .. 4 l + 3
            const int4 h = *reinterpret_cast<const int4 *>(hist + 4 * lane);
            const int own = h.x + h.y + h.z + h.w;
            int suf = own;                                  // the keys whose digit is >= 4 l
#pragma unroll
            for (int off = 1; off < kWave; off <<= 1) {
                const int t = __shfl_down(suf, off, kWave);
                if (lane + off < kWave) suf += t;
            }
            const int above = suf - own;
            const bool mine = above < krem && krem <= suf;
            int digit = 0, left = krem;
            if (mine) {
                int acc = above;
                const int hh[4] = {h.x, h.y, h.z, h.w};
                digit = 4 * lane;
                left = krem - acc;
#pragma unroll
                for (int d = 3; d >= 0; --d) {
                    if (acc + hh[d] >= krem) { digit = 4 * lane + d; left = krem - acc; break; }
                    acc += hh[d];
                }
            }
            const unsigned long long mm = __ballot(mine);
            const int src = mm ? __ffsll((long long)mm) - 1 : 0;
            digit = __shfl(digit, src, kWave);
            krem = __shfl(left, src, kWave);
            prefix |= (uint32_t)digit << shift;
        }
        // prefix: the key of the keff-th largest weight; krem of the entries with that key are taken, lowest rows first.
        // Zeros are never stored (KNNCFRecommender.py:351): when the threshold is the zero key nothing equal to it is kept.
        const uint32_t thr = prefix;
        const int take_eq = thr == kKnnZeroKey ? 0 : krem;
        int32_t *out_row = rows + j * K;
        float *out_val = vals + j * K;
        int run_gt = 0, run_eq = 0, par = 0;
        for (int64_t base = 0; base < n; base += kBlock) {
            const int64_t i = base + tid;
            float w = 0.f;
            bool gt = false, eq = false;
            if (i < n) {
                w = knn_weight(p, g[i], ss[i], i == j);
                const uint32_t key = knn_key(w);
                gt = key > thr && key != kKnnZeroKey;
                eq = key == thr;
            }
            const unsigned long long gm = __ballot(gt), em = __ballot(eq);
            if (lane == 0) { s_cnt[par][wave][0] = __popcll(gm); s_cnt[par][wave][1] = __popcll(em); }
            __syncthreads();
            int gt_before = run_gt + __popcll(gm & below), eq_before = run_eq + __popcll(em & below);
            int gt_all = 0, eq_all = 0;
#pragma unroll
            for (int wv = 0; wv < kKnnWaves; ++wv) {
                const int cg = s_cnt[par][wv][0], ce = s_cnt[par][wv][1];
                if (wv < wave) { gt_before += cg; eq_before += ce; }
                gt_all += cg;
                eq_all += ce;
            }
            par ^= 1;
            if (gt || (eq && eq_before < take_eq)) {
                const int slot = gt_before + (eq_before < take_eq ? eq_before : take_eq);
                if (slot < K) { out_row[slot] = (int32_t)i; out_val[slot] = w; }      // (always: slot < keff <= K)
            }
            run_gt += gt_all;
            run_eq += eq_all;
        }
        const int kept = run_gt + (run_eq < take_eq ? run_eq : take_eq);
        for (int sidx = kept + tid; sidx < K; sidx += kBlock) { out_row[sidx] = -1; out_val[sidx] = 0.f; }
        if (tid == 0) count[j] = kept;
        __syncthreads();                                    // s_hist is zeroed again for the next column
    }
}

// ---- scores and top-k ------------------------------------------------------------------------------------------------
// One workgroup per requested row of L, a thread per candidate column of R; the products of two fp32 values are exact in
// fp64, the sum runs over the column's entries in ascending k.
template <bool LDS>
__global__ __launch_bounds__(kBlock) void k_knn_rank(const int64_t *__restrict__ l_ptr, const int32_t *__restrict__ l_col,
                                                     const float *__restrict__ l_val, int64_t n_rows, int64_t inner,
                                                     const int64_t *__restrict__ r_ptr, const int32_t *__restrict__ r_row,
                                                     const float *__restrict__ r_val, int64_t n_cols,
                                                     const int64_t *__restrict__ users, const int64_t *__restrict__ items,
                                                     int64_t C, int topk, double *scores, int64_t *__restrict__ out_ids) {
    extern __shared__ __attribute__((aligned(16))) float knn_x[];
    const int64_t b = blockIdx.x;
    const int64_t u = users[b];
    const bool valid = u >= 0 && u < n_rows;
    const int64_t beg = valid ? l_ptr[u] : 0, end = valid ? l_ptr[u + 1] : 0;
    if (LDS) sparse_row_to_lds(knn_x, inner, l_col, l_val, beg, end);
    double *row = scores + b * C;
    for (int64_t c = threadIdx.x; c < C; c += kBlock) {
        const int64_t it = items ? items[b * C + c] : c;
        double s = 0.0;
        if (valid && it >= 0 && it < n_cols)
            s = sparse_dot_score<LDS>(knn_x, l_col, l_val, beg, end, inner, r_ptr, r_row, r_val, it);
        row[c] = s;
    }
    if (!out_ids) return;
    topk_f64_select(row, C, topk, items ? items + b * C : nullptr, out_ids + b * topk);
}

}  // namespace
}  // namespace daisy

using namespace daisy;

extern "C" {

int daisy_knn_row_means(const int64_t *row_ptr, const float *val, int64_t n_rows, float *mean, daisy_stream_t stream) {
    DAISY_CHECK_ARG(row_ptr && val && mean, "knn_row_means: NULL argument");
    DAISY_CHECK_ARG(n_rows >= 0 && n_rows <= INT_MAX, "knn_row_means: n_rows=%lld", (long long)n_rows);
    if (n_rows == 0) return DAISY_OK;
    hipLaunchKernelGGL(k_knn_row_means, dim3(grid_for(n_rows, kKnnWaves)), dim3(kBlock), 0, as_stream(stream), row_ptr, val,
                       n_rows, mean);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_knn_center(const int64_t *row_ptr, const int32_t *col, const float *val, int64_t n_rows, int64_t n_cols,
                     int32_t mode, const float *mean, float *out, daisy_stream_t stream) {
    DAISY_CHECK_ARG(row_ptr && col && val && out, "knn_center: NULL argument");
    DAISY_CHECK_ARG(n_rows >= 0 && n_rows <= INT_MAX && n_cols >= 1 && n_cols <= INT_MAX, "knn_center: n_rows=%lld n_cols=%lld",
                    (long long)n_rows, (long long)n_cols);
    DAISY_CHECK_ARG(mode >= DAISY_KNN_CENTER_NONE && mode <= DAISY_KNN_CENTER_BINARY, "knn_center: mode=%d", mode);
    DAISY_CHECK_ARG(mean || mode == DAISY_KNN_CENTER_NONE || mode == DAISY_KNN_CENTER_BINARY,
                    "knn_center: mode %d needs the means (NULL mean)", mode);
    if (n_rows == 0) return DAISY_OK;
    hipLaunchKernelGGL(k_knn_center, dim3(grid_for(n_rows, 1)), dim3(kBlock), 0, as_stream(stream), row_ptr, col, val, n_rows,
                       n_cols, (int)mode, mean, out);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_knn_diag(const float *G, int64_t n, int32_t take_sqrt, float *ss, daisy_stream_t stream) {
    DAISY_CHECK_ARG(G && ss, "knn_diag: NULL argument");
    DAISY_CHECK_ARG(n >= 1 && n <= INT_MAX, "knn_diag: n=%lld", (long long)n);
    hipLaunchKernelGGL(k_knn_diag, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, as_stream(stream), G, n, (int)(take_sqrt != 0),
                       ss);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_knn_select(const float *G, const float *ss, int64_t n, int32_t mode, float shrink, float alpha, int32_t K,
                     int32_t *count, int32_t *rows, float *vals, daisy_stream_t stream) {
    DAISY_CHECK_ARG(G && ss && count && rows && vals, "knn_select: NULL argument");
    DAISY_CHECK_ARG(n >= 1 && n <= INT_MAX, "knn_select: n=%lld", (long long)n);
    DAISY_CHECK_ARG(knn_mode_ok(mode), "knn_select: mode=%d", mode);
    DAISY_CHECK_ARG(shrink >= 0.f && shrink < INFINITY, "knn_select: shrink=%g must be finite and >= 0", (double)shrink);
    DAISY_CHECK_ARG(alpha >= 0.f && alpha <= 1.f, "knn_select: alpha=%g outside [0, 1]", (double)alpha);
    DAISY_CHECK_ARG(K >= 1 && K <= DAISY_KNN_MAX_K, "knn_select: K=%d outside [1, %d]", K, DAISY_KNN_MAX_K);
    if (mode == DAISY_KNN_ASYMMETRIC && alpha == 0.5f) mode = DAISY_KNN_COSINE;      // ss^1 * ss^1: cosine's own path
    hipLaunchKernelGGL(k_knn_select, dim3(grid_for(n, 1)), dim3(kBlock), 0, as_stream(stream), G, ss, n, (int)mode, shrink,
                       alpha, (int)K, count, rows, vals);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_knn_rank(const int64_t *l_ptr, const int32_t *l_col, const float *l_val, int64_t n_rows, int64_t inner,
                   const int64_t *r_ptr, const int32_t *r_row, const float *r_val, int64_t n_cols, const int64_t *users,
                   int64_t B, const int64_t *items, int64_t C, int32_t topk, double *scores, int64_t *out_ids, int32_t path,
                   daisy_stream_t stream) {
    DAISY_CHECK_ARG(l_ptr && l_col && l_val && r_ptr && r_row && r_val && scores, "knn_rank: NULL argument");
    DAISY_CHECK_ARG(n_rows >= 1 && inner >= 1 && inner <= INT_MAX && n_cols >= 1 && n_cols <= INT_MAX,
                    "knn_rank: n_rows=%lld inner=%lld n_cols=%lld", (long long)n_rows, (long long)inner, (long long)n_cols);
    DAISY_CHECK_ARG(B >= 0 && B <= INT_MAX && (B == 0 || users), "knn_rank: B=%lld users (NULL users?)", (long long)B);
    DAISY_CHECK_ARG(items ? C >= 1 : C == n_cols, "knn_rank: C=%lld candidates per user (n_cols when items == NULL)",
                    (long long)C);
    DAISY_CHECK_ARG(!out_ids || (topk >= 1 && topk <= C), "knn_rank: topk=%d outside [1, C=%lld]", topk, (long long)C);
    DAISY_CHECK_ARG(path >= DAISY_SLIM_PATH_AUTO && path <= DAISY_SLIM_PATH_GLOBAL, "knn_rank: path=%d", path);
    const bool lds = path == DAISY_SLIM_PATH_LDS || (path == DAISY_SLIM_PATH_AUTO && inner <= kKnnRankLdsItems);
    DAISY_CHECK_ARG(!lds || inner <= kKnnRankLdsItems, "knn_rank: the LDS path holds at most %d entries (inner=%lld)",
                    kKnnRankLdsItems, (long long)inner);
    if (B == 0) return DAISY_OK;
    hipStream_t s = as_stream(stream);
    if (lds) {
        DAISY_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_knn_rank<true>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, kKnnRankLdsItems * (int)sizeof(float)));
        hipLaunchKernelGGL(k_knn_rank<true>, dim3((unsigned)B), dim3(kBlock), (size_t)inner * sizeof(float), s, l_ptr, l_col,
                           l_val, n_rows, inner, r_ptr, r_row, r_val, n_cols, users, items, C, (int)topk, scores, out_ids);
    } else {
        hipLaunchKernelGGL(k_knn_rank<false>, dim3((unsigned)B), dim3(kBlock), 0, s, l_ptr, l_col, l_val, n_rows, inner, r_ptr,
                           r_row, r_val, n_cols, users, items, C, (int)topk, scores, out_ids);
    }
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

size_t daisy_knn_fit_bytes(int64_t n_rows, int64_t n, int32_t K) {
    if (n_rows < 0 || n < 1 || n > INT_MAX || K < 1 || K > DAISY_KNN_MAX_K) return 0;
    return align_up((size_t)n * (size_t)n * sizeof(float)) + daisy_slim_gram_workspace_bytes(n_rows, n, 0) + knn_out_bytes(n, K);
}

int daisy_knn_fits(int64_t n_rows, int64_t n, int32_t K, size_t offered_bytes) {
    DAISY_CHECK_ARG(n_rows >= 0 && n >= 1 && n <= INT_MAX, "knn_fits: n_rows=%lld n=%lld", (long long)n_rows, (long long)n);
    DAISY_CHECK_ARG(K >= 1 && K <= DAISY_KNN_MAX_K, "knn_fits: K=%d outside [1, %d]", K, DAISY_KNN_MAX_K);
    const size_t g = align_up((size_t)n * (size_t)n * sizeof(float));
    const size_t ws = daisy_slim_gram_workspace_bytes(n_rows, n, 0), out = knn_out_bytes(n, K);
    DAISY_CHECK_ARG(daisy_knn_fit_bytes(n_rows, n, K) <= offered_bytes,
                    "knn_fits: G [%lld x %lld] fp32 (%zu bytes), the Gram workspace (%zu bytes) and the kept neighbours with "
                    "the norms (%zu bytes) take %zu bytes: that does not fit the %zu bytes offered",
                    (long long)n, (long long)n, g, ws, out, g + ws + out, offered_bytes);
    return DAISY_OK;
}

}  // extern "C"
