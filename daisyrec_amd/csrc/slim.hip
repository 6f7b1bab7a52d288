// SLiM (daisy/model/SLiMRecommender.py): the Gram matrix G = X^T X on the fp32 MFMA product, one
// non-negative elastic net per item column by cyclic coordinate descent over G (fp64 state, one workgroup per column,
// columns handed out by an atomic counter), the reference's top-k truncation, and the rows of A_tilde = X W.
#include <limits.h>

#include "common.h"
#include "gemm.h"
#include "score_f64.h"

namespace daisy {
namespace {

constexpr int kSlimTileRowsMax = 1024;                                     // user rows densified per product
constexpr size_t kSlimCdLdsBytes = (size_t)DAISY_SLIM_LDS_ITEMS * 16;      // w + H of one column: 156 of the 160 KB
constexpr int kSlimScoreLdsItems = 32768;                                  // a user's dense row of X: 128 KB
constexpr int kSlimWaves = kBlock / kWave;

inline size_t slim_partial_bytes(int64_t I) { return align_up((size_t)I * (size_t)I * sizeof(float)); }
inline int64_t slim_tile_rows(int64_t user_num, int64_t tile_rows) {
    int64_t r = tile_rows > 0 ? tile_rows : kSlimTileRowsMax;
    const int64_t need = user_num > 1 ? user_num : 1;
    if (tile_rows <= 0 && r > need) r = need;
    return (r + 15) / 16 * 16;
}

// ---- Gram ------------------------------------------------------------------------------------------------------------
// rows [u0, u0 + rows) of X into the zeroed tile [*, I]: one workgroup per row at a time
__global__ __launch_bounds__(kBlock) void k_slim_densify(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                         const float *__restrict__ val, int64_t u0, int64_t rows, int64_t I,
                                                         float *__restrict__ tile) {
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const int64_t beg = row_ptr[u0 + r], end = row_ptr[u0 + r + 1];
        for (int64_t e = beg + threadIdx.x; e < end; e += kBlock) {
            const int32_t c = col[e];
            if (c >= 0 && c < I) tile[r * I + c] = val[e];
        }
    }
}

// G += P, element by element: the user blocks' products are added in block order
__global__ __launch_bounds__(kBlock) void k_slim_add(const float *__restrict__ P, float *__restrict__ G, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) G[i] += P[i];
}

__global__ __launch_bounds__(kBlock) void k_slim_diag(const float *__restrict__ G, int64_t I, float *__restrict__ diag) {
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < I; i += (int64_t)gridDim.x * kBlock) diag[i] = G[i * I + i];
}

// ---- coordinate descent ----------------------------------------------------------------------------------------------
// From here on no multiply-add is contracted: the descent's update sequence is that of the plain fp64 rule, operation by
// operation, so it can be checked against a numpy transcription almost bit for bit (the scores' products are exact).
#pragma clang fp contract(off)
struct SlimCdArgs {
    const float *G;
    const float *diag;
    int I;
    double a, b, tol;
    int max_iter, topk;
    int64_t col0;
    int ncols;
    int *counter;
    int32_t *kept_count, *kept_row;
    float *kept_val;
    int32_t *sweeps;
    double *gap;
    int64_t *moves;         // may be NULL
    double *state;          // global path: w and H of workgroup g at state + g * 2 * I
};

// The reductions of a workgroup: every thread gets the result, waves combined in wave order (one barrier; the slot
// parity alternates so that the next reduction may start while slow waves still read this one's).
struct SlimRed {
    double v[2][kSlimWaves][5];
    int i[2][kSlimWaves];
};

__device__ __forceinline__ double wave_max_f64(double x) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) x = fmax(x, __shfl_xor(x, off, kWave));
    return x;
}

// Cyclic coordinate descent of one column per workgroup turn.  Within a sweep, H[i] and w[i] are only ever touched by
// thread i % kBlock, so a sweep needs no barrier but the one that publishes the coordinate that moved.
template <bool LDS>
__global__ __launch_bounds__(kBlock) void k_slim_cd(SlimCdArgs p) {
    extern __shared__ __attribute__((aligned(16))) double slim_state[];
    __shared__ SlimRed red;
    __shared__ int s_col;
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const int I = p.I;
    double *w = LDS ? slim_state : p.state + (int64_t)blockIdx.x * 2 * I;
    double *H = w + I;
    int par = 0;                      // parity of the exchange slots (uniform)

    // (value, index) of the first wave lane / the first wave with flag set; kBlock when none
    auto first_moved = [&](bool moved, double delta, double &delta_out) -> int {
        const unsigned long long m = __ballot(moved);
        const int f = m ? (__ffsll((long long)m) - 1) : -1;
        if (lane == (f < 0 ? 0 : f)) {
            red.i[par][wave] = f < 0 ? kBlock : wave * kWave + f;
            red.v[par][wave][0] = delta;
        }
        __syncthreads();
        int first = kBlock;
        double d = 0.0;
#pragma unroll
        for (int wv = kSlimWaves - 1; wv >= 0; --wv) {
            const int fi = red.i[par][wv];
            if (fi < kBlock) { first = fi; d = red.v[par][wv][0]; }
        }
        par ^= 1;
        delta_out = d;
        return first;
    };
    auto block_sums = [&](double (&x)[5], int nsum) {          // x[0 .. nsum) summed, x[4] maximised
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < nsum) x[k] = wave_sum_f64(x[k]);
        x[4] = wave_max_f64(x[4]);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 5; ++k) red.v[par][wave][k] = x[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            double t = red.v[par][0][k];
#pragma unroll
            for (int wv = 1; wv < kSlimWaves; ++wv) t = (k == 4) ? fmax(t, red.v[par][wv][k]) : t + red.v[par][wv][k];
            x[k] = t;
        }
        par ^= 1;
    };

    for (;;) {
        if (tid == 0) s_col = atomicAdd(p.counter, 1);
        __syncthreads();
        const int cj = s_col;
        __syncthreads();
        if (cj >= p.ncols) return;
        const int j = (int)(p.col0 + cj);
        const float *__restrict__ q = p.G + (int64_t)j * I;      // G is symmetric: column j is the contiguous row j
        const double yy = (double)p.diag[j];
        int32_t *out_row = p.kept_row + (int64_t)cj * p.topk;
        float *out_val = p.kept_val + (int64_t)cj * p.topk;

        int n_sweeps = 0, keep = 0;
        int64_t n_moves = 0;
        double gap = 0.0;
        if (yy != 0.0) {
            for (int i = tid; i < I; i += kBlock) { w[i] = 0.0; H[i] = 0.0; }
            for (int it = 0; it < p.max_iter; ++it) {
                double d_w_max = 0.0;
                for (int base = 0; base < I; base += kBlock) {
                    const int k = base + tid;
                    const bool elig = k < I && k != j;
                    const double d = elig ? (double)p.diag[k] : 0.0;
                    const double qk = elig ? (double)q[k] : 0.0;
                    const bool active = elig && d != 0.0;          // Q[k,k] == 0: skipped (k == j, unrated items)
                    int start = 0;
                    for (;;) {
                        // Every lane from `start` on evaluates its coordinate against the current H.  A coordinate whose
                        // value does not change leaves H untouched, so up to the first lane that moves this IS the
                        // sequential sweep; that lane's update is applied by everyone and the lanes after it look again.
                        bool moved = false;
                        double wn = 0.0, wo = 0.0;
                        if (active && tid >= start) {
                            wo = w[k];
                            const double t = qk - (H[k] - wo * d);
                            wn = (t < 0.0) ? 0.0 : fmax(t - p.a, 0.0) / (d + p.b);
                            moved = (wn != wo);
                        }
                        double delta;
                        const int f = first_moved(moved, wn - wo, delta);
                        if (f >= kBlock) break;
                        if (tid == f) w[k] = wn;
                        const float *__restrict__ row = p.G + (int64_t)(base + f) * I;
                        for (int i = tid; i < I; i += kBlock)
                            if (i != j) H[i] += delta * (double)row[i];
                        d_w_max = fmax(d_w_max, fabs(delta));
                        ++n_moves;
                        start = f + 1;
                    }
                }
                n_sweeps = it + 1;
                double x[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
                for (int i = tid; i < I; i += kBlock) x[4] = fmax(x[4], fabs(w[i]));
                block_sums(x, 0);
                const double w_max = x[4];
                if (w_max == 0.0 || d_w_max / w_max < p.tol || it == p.max_iter - 1) {
                    // the duality gap (positive=True: the maximum of XtA, not of its modulus; entry j of XtA is 0)
                    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
                    for (int i = tid; i < I; i += kBlock) {
                        const double wi = w[i], hi = H[i];
                        const double qi = (i == j) ? 0.0 : (double)q[i];
                        s[0] += wi * hi;
                        s[1] += qi * wi;
                        s[2] += fabs(wi);
                        s[3] += wi * wi;
                        s[4] = fmax(s[4], qi - hi - p.b * wi);
                    }
                    block_sums(s, 4);
                    const double R = yy + s[0] - 2.0 * s[1];
                    double c = 1.0;
                    if (s[4] > p.a) {
                        c = p.a / s[4];
                        gap = 0.5 * R * (1.0 + c * c);
                    } else {
                        gap = R;
                    }
                    gap += p.a * s[2] - c * yy + c * s[1] + 0.5 * p.b * (1.0 + c * c) * s[3];
                    if (gap < p.tol * yy) break;
                }
            }
            // SLiMRecommender.py:86-107: the min(nz - 1, topk) largest coefficients, ties to the lower row
            double x[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
            for (int i = tid; i < I; i += kBlock) x[0] += (w[i] != 0.0) ? 1.0 : 0.0;
            block_sums(x, 1);
            const int nz = (int)x[0];
            keep = nz - 1 < p.topk ? nz - 1 : p.topk;
            if (keep < 0) keep = 0;
            for (int sel = 0; sel < keep; ++sel) {
                double bv = 0.0;
                int bi = INT_MAX;
                for (int i = tid; i < I; i += kBlock) {            // ascending i: the first maximum is the lowest row
                    const double v = w[i];
                    if (v > bv) { bv = v; bi = i; }
                }
#pragma unroll
                for (int off = kWave / 2; off > 0; off >>= 1) {
                    const double ov = __shfl_xor(bv, off, kWave);
                    const int oi = __shfl_xor(bi, off, kWave);
                    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
                }
                if (lane == 0) { red.v[par][wave][0] = bv; red.i[par][wave] = bi; }
                __syncthreads();
                bv = red.v[par][0][0];
                bi = red.i[par][0];
#pragma unroll
                for (int wv = 1; wv < kSlimWaves; ++wv) {
                    const double ov = red.v[par][wv][0];
                    const int oi = red.i[par][wv];
                    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
                }
                par ^= 1;
                if (bi == INT_MAX) { keep = sel; break; }          // (nothing positive left: not-a-number coefficients)
                if (tid == bi % kBlock) w[bi] = 0.0;               // taken (its owner thread is the only one that reads it)
                if (tid == 0) { out_row[sel] = bi; out_val[sel] = (float)bv; }
            }
        }
        for (int sidx = keep + tid; sidx < p.topk; sidx += kBlock) { out_row[sidx] = -1; out_val[sidx] = 0.f; }
        if (tid == 0) {
            p.kept_count[cj] = keep;
            p.sweeps[cj] = n_sweeps;
            p.gap[cj] = gap;
            if (p.moves) p.moves[cj] = n_moves;
        }
    }
}

// ---- scores ----------------------------------------------------------------------------------------------------------
template <bool LDS>
__global__ __launch_bounds__(kBlock) void k_slim_scores(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                        const float *__restrict__ val, int64_t U, int64_t I,
                                                        const int64_t *__restrict__ w_ptr, const int32_t *__restrict__ w_row,
                                                        const float *__restrict__ w_val, const int64_t *__restrict__ users,
                                                        const int64_t *__restrict__ items, int64_t C, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float slim_x[];
    const int64_t b = blockIdx.x;
    const int64_t u = users[b];
    const bool valid = u >= 0 && u < U;
    const int64_t beg = valid ? row_ptr[u] : 0, end = valid ? row_ptr[u + 1] : 0;
    if (LDS) sparse_row_to_lds(slim_x, I, col, val, beg, end);
    const int64_t width = items ? C : I;
    for (int64_t c = threadIdx.x; c < width; c += kBlock) {
        const int64_t it = items ? items[b * C + c] : c;
        double s = 0.0;
        if (valid && it >= 0 && it < I) s = sparse_dot_score<LDS>(slim_x, col, val, beg, end, I, w_ptr, w_row, w_val, it);
        out[b * width + c] = (float)s;
    }
}

int slim_cd_path(int64_t item_num, int32_t path) {
    if (path == DAISY_SLIM_PATH_AUTO) return item_num <= DAISY_SLIM_LDS_ITEMS ? DAISY_SLIM_PATH_LDS : DAISY_SLIM_PATH_GLOBAL;
    return path;
}

constexpr int kSlimCdMaxGroups = 2048;     // workgroups of the descent launch, state in LDS (256 CUs x at most 8)
// State in global memory: one workgroup per CU.  Each owns 16 bytes per item (160 KB and more), so 256 of them keep
// 41 MB+ of fp64 state in flight: about 5 MB per XCD, around the size of its 4 MB L2 - more workgroups would only push
// the read-modify-write of every H update out to the Infinity Cache.
constexpr int kSlimCdGlobalGroups = 256;

// workspace of the descent: [counter: 256 B][diag: I floats][state: groups x 2 x I doubles on the global path]
int64_t slim_cd_groups_cap(int64_t ncols, int use_path) {
    const int64_t cap = use_path == DAISY_SLIM_PATH_GLOBAL ? kSlimCdGlobalGroups : kSlimCdMaxGroups;
    return ncols < cap ? ncols : cap;
}

}  // namespace
}  // namespace daisy

using namespace daisy;

extern "C" {

size_t daisy_slim_gram_workspace_bytes(int64_t user_num, int64_t item_num, int64_t tile_rows) {
    if (item_num < 1 || item_num > INT_MAX || user_num < 0) return 0;
    return slim_partial_bytes(item_num) + align_up((size_t)slim_tile_rows(user_num, tile_rows) * (size_t)item_num * sizeof(float));
}

int daisy_slim_gram_fits(int64_t user_num, int64_t item_num, int64_t tile_rows, size_t offered_bytes) {
    DAISY_CHECK_ARG(user_num >= 0 && item_num >= 1 && item_num <= INT_MAX, "slim_gram: user_num=%lld item_num=%lld",
                    (long long)user_num, (long long)item_num);
    const size_t g = (size_t)item_num * (size_t)item_num * sizeof(float);
    const size_t ws = daisy_slim_gram_workspace_bytes(user_num, item_num, tile_rows);
    // (item_num <= INT_MAX: g < 2^64; the comparison is written so that g + ws cannot wrap)
    DAISY_CHECK_ARG(g <= offered_bytes && ws <= offered_bytes - g,
                    "slim_gram: G [%lld x %lld] fp32 (%zu bytes) plus the Gram workspace (%zu bytes) does not fit the %zu "
                    "bytes offered", (long long)item_num, (long long)item_num, g, ws, offered_bytes);
    return DAISY_OK;
}

int daisy_slim_gram(const int64_t *row_ptr, const int32_t *col, const float *val, int64_t user_num, int64_t item_num,
                    float *G, void *workspace, size_t workspace_bytes, daisy_stream_t stream) {
    DAISY_CHECK_ARG(row_ptr && G && workspace, "slim_gram: NULL argument");
    DAISY_CHECK_ARG(user_num >= 0 && item_num >= 1 && item_num <= INT_MAX, "slim_gram: user_num=%lld item_num=%lld",
                    (long long)user_num, (long long)item_num);
    DAISY_CHECK_ARG(col && val, "slim_gram: NULL col / val");
    const size_t pbytes = slim_partial_bytes(item_num);
    const size_t row_bytes = (size_t)item_num * sizeof(float);
    DAISY_CHECK_ARG(workspace_bytes >= pbytes + 16 * row_bytes,
                    "slim_gram: workspace of %zu bytes, need at least %zu (daisy_slim_gram_workspace_bytes)", workspace_bytes,
                    pbytes + 16 * row_bytes);
    int64_t R = (int64_t)((workspace_bytes - pbytes) / row_bytes);
    const int64_t want = slim_tile_rows(user_num, 0);
    if (R > want) R = want;
    R = R / 16 * 16;
    hipStream_t s = as_stream(stream);
    const int64_t I = item_num;
    float *partial = static_cast<float *>(workspace);
    float *tile = reinterpret_cast<float *>(static_cast<char *>(workspace) + pbytes);
    if (user_num == 0) {
        DAISY_HIP(hipMemsetAsync(G, 0, (size_t)I * I * sizeof(float), s));
        return DAISY_OK;
    }
    for (int64_t u0 = 0; u0 < user_num; u0 += R) {
        const int64_t rows = (user_num - u0 < R) ? user_num - u0 : R;
        const int64_t K = (rows + 15) / 16 * 16;                    // (zero rows up to the next multiple of 16)
        DAISY_HIP(hipMemsetAsync(tile, 0, (size_t)K * row_bytes, s));
        hipLaunchKernelGGL(k_slim_densify, dim3(grid_for(rows, 1)), dim3(kBlock), 0, s, row_ptr, col, val, u0, rows, I, tile);
        DAISY_LAUNCH_CHECK();
        // tile^T tile: A(m,k) = tile[k*I + m], B(n,k) = tile[k*I + n]
        gemm_f32(tile, 1, I, tile, 1, I, u0 == 0 ? G : partial, I, I, (int)I, K, K, 0, s);
        DAISY_LAUNCH_CHECK();
        if (u0 > 0) {
            hipLaunchKernelGGL(k_slim_add, dim3(grid_for(I * I, kBlock)), dim3(kBlock), 0, s, partial, G, I * I);
            DAISY_LAUNCH_CHECK();
        }
    }
    return DAISY_OK;
}

size_t daisy_slim_cd_workspace_bytes(int64_t item_num, int64_t ncols, int32_t path) {
    if (item_num < 1 || item_num > INT_MAX || ncols < 0 || ncols > item_num || path < DAISY_SLIM_PATH_AUTO ||
        path > DAISY_SLIM_PATH_GLOBAL)
        return 0;
    size_t b = 256 + align_up((size_t)item_num * sizeof(float));
    if (slim_cd_path(item_num, path) == DAISY_SLIM_PATH_GLOBAL)
        b += align_up((size_t)slim_cd_groups_cap(ncols, DAISY_SLIM_PATH_GLOBAL) * 2 * (size_t)item_num * sizeof(double));
    return b;
}

int daisy_slim_cd(const float *G, int64_t item_num, int64_t n_users, double alpha, double l1_ratio, double tol,
                  int32_t max_iter, int32_t topk, int64_t col0, int64_t ncols, int32_t *kept_count, int32_t *kept_row,
                  float *kept_val, int32_t *sweeps, double *gap, int64_t *moves, int32_t path, void *workspace,
                  size_t workspace_bytes, daisy_stream_t stream) {
    DAISY_CHECK_ARG(G && kept_count && kept_row && kept_val && sweeps && gap && workspace, "slim_cd: NULL argument");
    DAISY_CHECK_ARG(item_num >= 1 && item_num <= INT_MAX && n_users >= 0, "slim_cd: item_num=%lld n_users=%lld",
                    (long long)item_num, (long long)n_users);
    DAISY_CHECK_ARG(alpha > 0.0 && alpha < INFINITY, "slim_cd: alpha=%g must be positive", alpha);
    DAISY_CHECK_ARG(l1_ratio >= 0.0 && l1_ratio <= 1.0, "slim_cd: l1_ratio=%g outside [0, 1]", l1_ratio);
    DAISY_CHECK_ARG(tol >= 0.0 && tol < INFINITY, "slim_cd: tol=%g must be >= 0", tol);
    DAISY_CHECK_ARG(max_iter >= 1, "slim_cd: max_iter=%d must be >= 1", max_iter);
    DAISY_CHECK_ARG(topk >= 1 && topk <= DAISY_SLIM_MAX_TOPK, "slim_cd: topk=%d outside [1, %d]", topk, DAISY_SLIM_MAX_TOPK);
    DAISY_CHECK_ARG(col0 >= 0 && ncols >= 0 && col0 + ncols <= item_num, "slim_cd: columns [%lld, %lld) outside [0, %lld)",
                    (long long)col0, (long long)(col0 + ncols), (long long)item_num);
    DAISY_CHECK_ARG(path >= DAISY_SLIM_PATH_AUTO && path <= DAISY_SLIM_PATH_GLOBAL, "slim_cd: path=%d", path);
    const int use = slim_cd_path(item_num, path);
    DAISY_CHECK_ARG(use != DAISY_SLIM_PATH_LDS || item_num <= DAISY_SLIM_LDS_ITEMS,
                    "slim_cd: the LDS path holds at most %d items (item_num=%lld)", DAISY_SLIM_LDS_ITEMS, (long long)item_num);
    const size_t need = daisy_slim_cd_workspace_bytes(item_num, ncols, path);
    DAISY_CHECK_ARG(workspace_bytes >= need, "slim_cd: workspace of %zu bytes, need %zu (daisy_slim_cd_workspace_bytes)",
                    workspace_bytes, need);
    if (ncols == 0) return DAISY_OK;
    hipStream_t s = as_stream(stream);
    char *ws = static_cast<char *>(workspace);
    SlimCdArgs a{};
    a.G = G;
    a.counter = reinterpret_cast<int *>(ws);
    float *diag = reinterpret_cast<float *>(ws + 256);
    a.diag = diag;
    a.state = reinterpret_cast<double *>(ws + 256 + align_up((size_t)item_num * sizeof(float)));
    a.I = (int)item_num;
    a.a = alpha * l1_ratio * (double)n_users;
    a.b = alpha * (1.0 - l1_ratio) * (double)n_users;
    a.tol = tol;
    a.max_iter = max_iter;
    a.topk = topk;
    a.col0 = col0;
    a.ncols = (int)ncols;
    a.kept_count = kept_count; a.kept_row = kept_row; a.kept_val = kept_val; a.sweeps = sweeps; a.gap = gap; a.moves = moves;
    DAISY_HIP(hipMemsetAsync(a.counter, 0, 256, s));
    hipLaunchKernelGGL(k_slim_diag, dim3(grid_for(item_num, kBlock)), dim3(kBlock), 0, s, G, item_num, diag);
    DAISY_LAUNCH_CHECK();
    int64_t groups = slim_cd_groups_cap(ncols, use);
    if (use == DAISY_SLIM_PATH_LDS) {
        const size_t shmem = (size_t)item_num * 16;
        // as many workgroups as fit the CUs' LDS at once (160 KB each, at most 8 per CU): the rest only queue
        int dev = 0, cus = 0;
        DAISY_HIP(hipGetDevice(&dev));
        DAISY_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        int64_t per_cu = (int64_t)((160 * 1024) / (shmem + 1024));
        if (per_cu < 1) per_cu = 1;
        if (per_cu > 8) per_cu = 8;
        if (cus > 0 && groups > cus * per_cu) groups = cus * per_cu;
        DAISY_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_slim_cd<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)kSlimCdLdsBytes));
        hipLaunchKernelGGL(k_slim_cd<true>, dim3((unsigned)groups), dim3(kBlock), shmem, s, a);
    } else {
        hipLaunchKernelGGL(k_slim_cd<false>, dim3((unsigned)groups), dim3(kBlock), 0, s, a);
    }
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_slim_scores(const int64_t *row_ptr, const int32_t *col, const float *val, int64_t user_num, int64_t item_num,
                      const int64_t *w_ptr, const int32_t *w_row, const float *w_val, const int64_t *users, int64_t B,
                      const int64_t *items, int64_t C, float *out, int32_t path, daisy_stream_t stream) {
    DAISY_CHECK_ARG(row_ptr && col && val && w_ptr && w_row && w_val && out, "slim_scores: NULL argument");
    DAISY_CHECK_ARG(user_num >= 0 && item_num >= 1 && item_num <= INT_MAX, "slim_scores: user_num=%lld item_num=%lld",
                    (long long)user_num, (long long)item_num);
    DAISY_CHECK_ARG(B >= 0 && B <= INT_MAX && (B == 0 || users), "slim_scores: B=%lld users (NULL users?)", (long long)B);
    DAISY_CHECK_ARG(!items || C >= 1, "slim_scores: C=%lld candidates per user", (long long)C);
    DAISY_CHECK_ARG(path >= DAISY_SLIM_PATH_AUTO && path <= DAISY_SLIM_PATH_GLOBAL, "slim_scores: path=%d", path);
    const bool lds = path == DAISY_SLIM_PATH_LDS || (path == DAISY_SLIM_PATH_AUTO && item_num <= kSlimScoreLdsItems);
    DAISY_CHECK_ARG(!lds || item_num <= kSlimScoreLdsItems, "slim_scores: the LDS path holds at most %d items (item_num=%lld)",
                    kSlimScoreLdsItems, (long long)item_num);
    if (B == 0) return DAISY_OK;
    hipStream_t s = as_stream(stream);
    if (lds) {
        DAISY_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_slim_scores<true>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, kSlimScoreLdsItems * (int)sizeof(float)));
        hipLaunchKernelGGL(k_slim_scores<true>, dim3((unsigned)B), dim3(kBlock), (size_t)item_num * sizeof(float), s, row_ptr, col,
                           val, user_num, item_num, w_ptr, w_row, w_val, users, items, C, out);
    } else {
        hipLaunchKernelGGL(k_slim_scores<false>, dim3((unsigned)B), dim3(kBlock), 0, s, row_ptr, col, val, user_num, item_num,
                           w_ptr, w_row, w_val, users, items, C, out);
    }
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // extern "C"
