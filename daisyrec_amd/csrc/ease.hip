// EASE (daisy/model/EASERecommender.py): B = -P / diag(P) with a zero diagonal, P = (X^T X + reg I)^-1, in
// fp64.  The inverse is a blocked Cholesky factorisation A = L L^T (block 64, right-looking), the blocked inverse T = L^-1
// and the product P = T^T T, the dense products on the fp64 MFMA.  Every element's sum runs over k in ascending order in
// a workgroup fixed by the element's position: no atomics, no split-K, no kernel waits on another workgroup, every loop
// bound is a function of the shapes alone.  Matrices are row-major [n, n]; every element index is an int64.
//
// v_mfma_f64_16x16x4_f64 (as in puresvd.hip): lane l feeds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] and
// gets D[row = (l >> 4) + 4 reg][col = l & 15], reg 0..3.  Rows and columns past n are zeros in registers.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "score_f64.h"
#include "topk_f64.h"

namespace daisy {
namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int kNb = DAISY_EASE_BLOCK;              // the factorisation's block
constexpr int kLd = kNb + 1;                       // row pitch of a block in LDS (fp64: 2 banks per element)
constexpr int64_t kEaseMaxItems = (int64_t)1 << 21;   // grids of (n / 64)^2 workgroups; n^2 * 16 bytes stays far below 2^64
static_assert(kNb == 64 && kBlock == 256, "four waves of 16 rows make one block");

#define MFMA_F64(a, b, acc) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (acc), 0, 0, 0)

inline int64_t ease_blocks(int64_t n) { return (n + kNb - 1) / kNb; }
inline size_t ease_dinv_bytes(int64_t n) { return align_up((size_t)ease_blocks(n) * kNb * kNb * sizeof(double)); }
inline size_t ease_diag_bytes(int64_t n) { return align_up((size_t)n * sizeof(double)); }

// ---- A = (double) G32 + reg I ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ease_system(const float *__restrict__ G, int64_t n, double reg,
                                                        double *__restrict__ A) {
    const int64_t nn = n * n;
    for (int64_t e = blockIdx.x * (int64_t)kBlock + threadIdx.x; e < nn; e += (int64_t)gridDim.x * kBlock) {
        const int64_t i = e / n, j = e - i * n;
        A[e] = (double)G[e] + (i == j ? reg : 0.0);
    }
}

// ---- potrf (a): the diagonal block and its inverse -------------------------------------------------------------------------
// One workgroup.  The block's lower triangle sits in LDS (rows past n: the identity); right-looking, column j of L then
// the update of the columns after it, so an element's sum runs over j ascending.  Then X = L^-1 row by row the same way:
// X[j][c] = R[j][c] / l_jj, R[i][c] -= L[i][j] X[j][c] (i > j).  R / X live transposed in the block's unused upper triangle,
// X's diagonal in s_xd.  first bad pivot (not > 0, or not a number) -> *info, unless an earlier block has set it.
__global__ __launch_bounds__(kBlock) void k_ease_potrf_diag(double *A, int64_t n, int64_t k0, double *__restrict__ Dinv,
                                                            int32_t *info) {
    __shared__ double s[kNb * kLd];
    __shared__ double s_xd[kNb];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    const int nb = (int)((n - k0 < kNb) ? n - k0 : kNb);
    for (int e = tid; e < kNb * kNb; e += kBlock) {
        const int i = e / kNb, j = e % kNb;
        double v = 0.0;
        if (j <= i) v = (i < nb) ? A[(k0 + i) * n + k0 + j] : (i == j ? 1.0 : 0.0);
        s[i * kLd + j] = v;
    }
    if (tid == 0) s_bad = -1;
    __syncthreads();
    for (int j = 0; j < kNb; ++j) {
        const double d = s[j * kLd + j];
        __syncthreads();
        const double ljj = sqrt(d);
        if (tid == 0 && !(d > 0.0) && s_bad < 0) s_bad = j;          // (padding rows have d == 1)
        if (tid == j) s[j * kLd + j] = ljj;
        if (tid > j && tid < kNb) s[tid * kLd + j] /= ljj;
        __syncthreads();
        const int m = kNb - 1 - j;                                      // the rows and columns after j
        for (int e = tid; e < m * m; e += kBlock) {
            const int i = j + 1 + e / m, c = j + 1 + e % m;
            if (i >= c) s[i * kLd + c] -= s[i * kLd + j] * s[c * kLd + j];
        }
        __syncthreads();
    }
    for (int j = 0; j < kNb; ++j) {
        const double ljj = s[j * kLd + j];
        if (tid < j) s[tid * kLd + j] /= ljj;                           // X[j][tid] = R[j][tid] / l_jj
        if (tid == j) s_xd[j] = 1.0 / ljj;
        __syncthreads();
        const int m = kNb - 1 - j;                                      // the rows after j, times the columns 0..j
        for (int e = tid; e < m * (j + 1); e += kBlock) {
            const int c = e / m, i = j + 1 + e % m;
            const double x = (c == j) ? s_xd[j] : s[c * kLd + j];
            s[c * kLd + i] -= s[i * kLd + j] * x;                       // R[i][c] -= L[i][j] X[j][c]
        }
        __syncthreads();
    }
    for (int e = tid; e < kNb * kNb; e += kBlock) {
        const int i = e / kNb, c = e % kNb;
        if (c <= i && i < nb) A[(k0 + i) * n + k0 + c] = s[i * kLd + c];
        Dinv[e] = (c < i) ? s[c * kLd + i] : (c == i ? s_xd[i] : 0.0);
    }
    if (tid == 0 && s_bad >= 0 && *info == 0) *info = (int32_t)(k0 + s_bad + 1);
}

// ---- potrf (b): the panel L21 = A21 L11^-T ---------------------------------------------------------------------------------
// A wave owns 16 rows of the panel.  The 64 columns in four groups of 16: group g starts from A21's tile, loses the
// products of the groups before it with L11[g, t]^T on the MFMA (k ascending), then is solved against the 16 x 16 diagonal
// tile L11[g, g]^T column by column (a lane holds one column of four rows; the finished column m comes from its lane by a
// shuffle).  The solved groups are kept in LDS in the MFMA's A layout.  Substitution with a division, not a product with
// L11^-1: with an integer factor every intermediate is an integer and the panel is exact.
__global__ __launch_bounds__(kBlock) void k_ease_potrf_panel(double *A, int64_t n, int64_t k0) {
    __shared__ double s_x[(kBlock / kWave) * 16 * kLd];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int col = lane & 15, quad = lane >> 4;
    double *sx = s_x + wave * 16 * kLd;
    const int64_t r0 = k0 + kNb + (int64_t)blockIdx.x * kNb + 16 * wave;
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {
        const int64_t c0 = k0 + 16 * g;                        // the group's first column; also L11's row of the same index
        doublex4 acc;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t row = r0 + quad + 4 * reg;
            acc[reg] = row < n ? A[row * n + c0 + col] : 0.0;
        }
        for (int k = 0; k < 16 * g; k += 4) {
            const double a = -sx[col * kLd + k + quad];                     // X[i = col][k]
            const double b = A[(c0 + col) * n + k0 + k + quad];             // L11[16 g + j][k]
            acc = MFMA_F64(a, b, acc);
        }
#pragma unroll 1
        for (int m = 0; m < 16; ++m) {
            const double lmm = A[(c0 + m) * n + c0 + m];
            const double lcm = col > m ? A[(c0 + col) * n + c0 + m] : 0.0;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const double x = acc[reg] / lmm;
                const double xm = __shfl(x, (lane & 48) | m, kWave);
                if (col == m) acc[reg] = x;
                else if (col > m) acc[reg] -= xm * lcm;
            }
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t row = r0 + quad + 4 * reg;
            sx[(quad + 4 * reg) * kLd + 16 * g + col] = acc[reg];
            if (row < n) A[row * n + c0 + col] = acc[reg];
        }
        __syncthreads();
    }
}

// ---- potrf (c): A22 -= L21 L21^T over the lower tiles ----------------------------------------------------------------------
// Workgroup (bj, bi), bj <= bi, owns one 64 x 64 block of the trailing matrix; wave w its tile row w, whose 16 x 64 strip
// of L21 stays in registers for the four tiles.  Only elements on or below the diagonal are written.
__global__ __launch_bounds__(kBlock) void k_ease_potrf_update(double *A, int64_t n, int64_t k0) {
    const int bj = blockIdx.x, bi = blockIdx.y;
    if (bj > bi) return;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int col = lane & 15, quad = lane >> 4;
    const int64_t t0 = k0 + kNb;
    const int64_t rt = t0 + (int64_t)bi * kNb + 16 * wave;
    const int64_t arow = rt + col;
    double a[16];
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) a[kk] = arow < n ? -A[arow * n + k0 + 4 * kk + quad] : 0.0;
#pragma unroll 1
    for (int tc = 0; tc < 4; ++tc) {
        if (bi == bj && tc > wave) break;                      // (uniform over the wave)
        const int64_t cg = t0 + (int64_t)bj * kNb + 16 * tc + col;
        doublex4 acc;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t row = rt + quad + 4 * reg;
            acc[reg] = (row < n && cg < n) ? A[row * n + cg] : 0.0;
        }
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const double b = cg < n ? A[cg * n + k0 + 4 * kk + quad] : 0.0;
            acc = MFMA_F64(a[kk], b, acc);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t row = rt + quad + 4 * reg;
            if (row < n && cg <= row) A[row * n + cg] = acc[reg];
        }
    }
}

// ---- potri, first half: block row bi of T = L^-1 ---------------------------------------------------------------------------
// T[bi, bi] = Dinv[bi];  T[bi, j] = -Dinv[bi] (sum_{k = j}^{bi - 1} L[bi, k] T[k, j]) for j < bi: the block rows above are
// complete (earlier launches).  Workgroup (strip, j) owns 16 columns of block column j: wave w sums its 16 x 16 tile of S
// over k ascending, the 64 x 16 strip of S meets in LDS, wave w multiplies its 16 rows of Dinv[bi] with it.
__global__ __launch_bounds__(kBlock) void k_ease_trtri_row(const double *__restrict__ L, const double *__restrict__ Dinv,
                                                           int64_t n, int bi, double *T) {
    __shared__ double s_s[kNb * 17];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int col = lane & 15, quad = lane >> 4;
    const int strip = blockIdx.x, j = blockIdx.y;
    const int64_t i0 = (int64_t)bi * kNb;
    const double *__restrict__ D = Dinv + (int64_t)bi * kNb * kNb;
    if (j == bi) {                                              // the diagonal block, zeros above the diagonal included
        for (int e = threadIdx.x; e < kNb * 16; e += kBlock) {
            const int r = e / 16, c = 16 * strip + e % 16;
            if (i0 + r < n && i0 + c < n) T[(i0 + r) * n + i0 + c] = D[r * kNb + c];
        }
        return;
    }
    const int64_t j0 = (int64_t)j * kNb + 16 * strip;          // (< i0 <= n: no column guard)
    const int64_t arow = i0 + 16 * wave + col;
    doublex4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int64_t k = (int64_t)j * kNb; k < i0; k += 4) {
        const double a = arow < n ? L[arow * n + k + quad] : 0.0;
        const double b = T[(k + quad) * n + j0 + col];
        acc = MFMA_F64(a, b, acc);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) s_s[(16 * wave + quad + 4 * reg) * 17 + col] = acc[reg];
    __syncthreads();
    doublex4 out = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kNb; k += 4) {
        const double a = -D[(16 * wave + col) * kNb + k + quad];
        const double b = s_s[(k + quad) * 17 + col];
        out = MFMA_F64(a, b, out);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int64_t row = i0 + 16 * wave + quad + 4 * reg;
        if (row < n) T[row * n + j0 + col] = out[reg];
    }
}

// ---- potri, second half: P = T^T T ------------------------------------------------------------------------------------------
// Workgroup (bj, bi), bi <= bj, owns one 64 x 64 block of the upper triangle; wave w its tile row w.  P[i][j] = sum over
// k >= 64 bj of T[k][i] T[k][j], k ascending (T's block rows above hold nothing for column j; inside the diagonal block
// the zeros above the diagonal are stored).  Every element on or above the diagonal is written to (i, j) and (j, i).
__global__ __launch_bounds__(kBlock) void k_ease_ttt(const double *__restrict__ T, int64_t n, double *__restrict__ P) {
    const int bj = blockIdx.x, bi = blockIdx.y;
    if (bi > bj) return;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int col = lane & 15, quad = lane >> 4;
    const int64_t ca = (int64_t)bi * kNb + 16 * wave + col;             // the A operand's column of T
    const int64_t cb0 = (int64_t)bj * kNb + col;
    const int first = (bi == bj) ? wave : 0;                           // tiles left of the diagonal tile are mirrored ones
    doublex4 acc[4];
#pragma unroll
    for (int tc = 0; tc < 4; ++tc) acc[tc] = doublex4{0.0, 0.0, 0.0, 0.0};
    for (int64_t k = (int64_t)bj * kNb; k < n; k += 4) {
        const int64_t kr = k + quad;
        const bool vk = kr < n;
        const double a = (vk && ca < n) ? T[kr * n + ca] : 0.0;
#pragma unroll
        for (int tc = 0; tc < 4; ++tc) {
            if (tc >= first) {
                const int64_t cb = cb0 + 16 * tc;
                const double b = (vk && cb < n) ? T[kr * n + cb] : 0.0;
                acc[tc] = MFMA_F64(a, b, acc[tc]);
            }
        }
    }
#pragma unroll
    for (int tc = 0; tc < 4; ++tc) {
        if (tc < first) continue;
        const int64_t cg = cb0 + 16 * tc;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t row = (int64_t)bi * kNb + 16 * wave + quad + 4 * reg;
            if (cg < n && row <= cg) {                                 // (row <= cg < n)
                P[row * n + cg] = acc[tc][reg];
                P[cg * n + row] = acc[tc][reg];
            }
        }
    }
}

// ---- B = -P / diag(P), zero diagonal -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ease_diag(const double *__restrict__ P, int64_t n, double *__restrict__ d) {
    for (int64_t j = blockIdx.x * (int64_t)kBlock + threadIdx.x; j < n; j += (int64_t)gridDim.x * kBlock) d[j] = P[j * n + j];
}

__global__ __launch_bounds__(kBlock) void k_ease_weights(const double *P, const double *__restrict__ d, int64_t n, double *B) {
    const int64_t nn = n * n;
    for (int64_t e = blockIdx.x * (int64_t)kBlock + threadIdx.x; e < nn; e += (int64_t)gridDim.x * kBlock) {
        const int64_t i = e / n, j = e - i * n;
        B[e] = (i == j) ? 0.0 : -P[e] / d[j];
    }
}

// ---- scores and top-k ---------------------------------------------------------------------------------------------------------
// One workgroup per user row, a thread per candidate: the user's CSR entries in stored order.  With items == NULL
// neighbouring threads read neighbouring columns of a history row of W.
__global__ __launch_bounds__(kBlock) void k_ease_rank(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                      const float *__restrict__ val, const double *__restrict__ W, int64_t U,
                                                      int64_t I, const int64_t *__restrict__ users,
                                                      const int64_t *__restrict__ items, int64_t C, int topk, double *scores,
                                                      int64_t *__restrict__ out_ids) {
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t u = users[b];
    const bool valid = u >= 0 && u < U;
    const int64_t beg = valid ? row_ptr[u] : 0, end = valid ? row_ptr[u + 1] : 0;
    double *row = scores + b * C;
    for (int64_t cidx = tid; cidx < C; cidx += kBlock) {
        const int64_t it = items ? items[b * C + cidx] : cidx;
        double s = 0.0;
        if (it >= 0 && it < I) s = ease_score(col, val, beg, end, W, I, it);
        row[cidx] = s;
    }
    if (!out_ids) return;
    topk_f64_select(row, C, topk, items ? items + b * C : nullptr, out_ids + b * topk);
}

}  // namespace
}  // namespace daisy

using namespace daisy;

extern "C" {

size_t daisy_ease_workspace_bytes(int64_t item_num) {
    if (item_num < 1 || item_num > kEaseMaxItems) return 0;
    return ease_dinv_bytes(item_num) + ease_diag_bytes(item_num);
}

size_t daisy_ease_fit_bytes(int64_t item_num) {
    if (item_num < 1 || item_num > kEaseMaxItems) return 0;
    return 2 * align_up((size_t)item_num * (size_t)item_num * sizeof(double)) + daisy_ease_workspace_bytes(item_num);
}

int daisy_ease_fits(int64_t item_num, size_t offered_bytes) {
    DAISY_CHECK_ARG(item_num >= 1 && item_num <= kEaseMaxItems, "ease_fits: item_num=%lld outside [1, %lld]",
                    (long long)item_num, (long long)kEaseMaxItems);
    const size_t need = daisy_ease_fit_bytes(item_num);
    DAISY_CHECK_ARG(need <= offered_bytes,
                    "ease_fits: two fp64 [%lld x %lld] buffers (the system, then L, P and B in place; and L^-1) plus the "
                    "workspace take %zu bytes at the peak: that does not fit the %zu bytes offered",
                    (long long)item_num, (long long)item_num, need, offered_bytes);
    return DAISY_OK;
}

int daisy_ease_system(const float *G, int64_t item_num, double reg, double *A, daisy_stream_t stream) {
    DAISY_CHECK_ARG(G && A, "ease_system: NULL argument");
    DAISY_CHECK_ARG(item_num >= 1 && item_num <= kEaseMaxItems, "ease_system: item_num=%lld outside [1, %lld]",
                    (long long)item_num, (long long)kEaseMaxItems);
    DAISY_CHECK_ARG(reg == reg, "ease_system: reg is not a number");
    hipLaunchKernelGGL(k_ease_system, dim3(grid_for(item_num * item_num, kBlock)), dim3(kBlock), 0, as_stream(stream), G,
                       item_num, reg, A);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_ease_potrf(double *A, int64_t n, int32_t *info, void *workspace, size_t workspace_bytes, daisy_stream_t stream) {
    DAISY_CHECK_ARG(A && info && workspace, "ease_potrf: NULL argument");
    DAISY_CHECK_ARG(n >= 1 && n <= kEaseMaxItems, "ease_potrf: n=%lld outside [1, %lld]", (long long)n,
                    (long long)kEaseMaxItems);
    const size_t need = daisy_ease_workspace_bytes(n);
    DAISY_CHECK_ARG(workspace_bytes >= need, "ease_potrf: workspace of %zu bytes, need %zu (daisy_ease_workspace_bytes)",
                    workspace_bytes, need);
    hipStream_t s = as_stream(stream);
    double *Dinv = static_cast<double *>(workspace);
    DAISY_HIP(hipMemsetAsync(info, 0, sizeof(int32_t), s));
    const int64_t nblk = ease_blocks(n);
    for (int64_t kb = 0; kb < nblk; ++kb) {
        const int64_t k0 = kb * kNb;
        hipLaunchKernelGGL(k_ease_potrf_diag, dim3(1), dim3(kBlock), 0, s, A, n, k0, Dinv + kb * kNb * kNb, info);
        DAISY_LAUNCH_CHECK();
        const int64_t below = nblk - kb - 1;                   // blocks of rows under the diagonal block
        if (below == 0) break;
        hipLaunchKernelGGL(k_ease_potrf_panel, dim3((unsigned)below), dim3(kBlock), 0, s, A, n, k0);
        DAISY_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_ease_potrf_update, dim3((unsigned)below, (unsigned)below), dim3(kBlock), 0, s, A, n, k0);
        DAISY_LAUNCH_CHECK();
    }
    return DAISY_OK;
}

int daisy_ease_potri(const double *L, int64_t n, double *T, double *P, const void *workspace, size_t workspace_bytes,
                     daisy_stream_t stream) {
    DAISY_CHECK_ARG(L && T && P && workspace, "ease_potri: NULL argument");
    DAISY_CHECK_ARG(n >= 1 && n <= kEaseMaxItems, "ease_potri: n=%lld outside [1, %lld]", (long long)n,
                    (long long)kEaseMaxItems);
    DAISY_CHECK_ARG(T != L && T != P, "ease_potri: T must be a buffer of its own (P may be L's)");
    const size_t need = daisy_ease_workspace_bytes(n);
    DAISY_CHECK_ARG(workspace_bytes >= need, "ease_potri: workspace of %zu bytes, need %zu (daisy_ease_workspace_bytes)",
                    workspace_bytes, need);
    hipStream_t s = as_stream(stream);
    const double *Dinv = static_cast<const double *>(workspace);
    const int64_t nblk = ease_blocks(n);
    for (int64_t bi = 0; bi < nblk; ++bi) {
        hipLaunchKernelGGL(k_ease_trtri_row, dim3(4, (unsigned)(bi + 1)), dim3(kBlock), 0, s, L, Dinv, n, (int)bi, T);
        DAISY_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_ease_ttt, dim3((unsigned)nblk, (unsigned)nblk), dim3(kBlock), 0, s, T, n, P);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_ease_weights(const double *P, int64_t n, double *B, void *workspace, size_t workspace_bytes,
                       daisy_stream_t stream) {
    DAISY_CHECK_ARG(P && B && workspace, "ease_weights: NULL argument");
    DAISY_CHECK_ARG(n >= 1 && n <= kEaseMaxItems, "ease_weights: n=%lld outside [1, %lld]", (long long)n,
                    (long long)kEaseMaxItems);
    const size_t need = daisy_ease_workspace_bytes(n);
    DAISY_CHECK_ARG(workspace_bytes >= need, "ease_weights: workspace of %zu bytes, need %zu (daisy_ease_workspace_bytes)",
                    workspace_bytes, need);
    hipStream_t s = as_stream(stream);
    double *d = reinterpret_cast<double *>(static_cast<char *>(workspace) + ease_dinv_bytes(n));
    hipLaunchKernelGGL(k_ease_diag, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, P, n, d);
    DAISY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ease_weights, dim3(grid_for(n * n, kBlock)), dim3(kBlock), 0, s, P, d, n, B);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_ease_rank(const int64_t *row_ptr, const int32_t *col, const float *val, const double *W, int64_t user_num,
                    int64_t item_num, const int64_t *users, int64_t B, const int64_t *items, int64_t C, int32_t topk,
                    double *scores, int64_t *out_ids, daisy_stream_t stream) {
    DAISY_CHECK_ARG(row_ptr && col && val && W && scores, "ease_rank: NULL argument");
    DAISY_CHECK_ARG(user_num >= 1 && item_num >= 1 && item_num <= kEaseMaxItems, "ease_rank: user_num=%lld item_num=%lld",
                    (long long)user_num, (long long)item_num);
    DAISY_CHECK_ARG(B >= 0 && B <= INT_MAX && (B == 0 || users), "ease_rank: B=%lld users (NULL users?)", (long long)B);
    DAISY_CHECK_ARG(items ? C >= 1 : C == item_num, "ease_rank: C=%lld candidates per user (item_num when items == NULL)",
                    (long long)C);
    DAISY_CHECK_ARG(!out_ids || (topk >= 1 && topk <= C), "ease_rank: topk=%d outside [1, C=%lld]", topk, (long long)C);
    if (B == 0) return DAISY_OK;
    hipLaunchKernelGGL(k_ease_rank, dim3((unsigned)B), dim3(kBlock), 0, as_stream(stream), row_ptr, col, val, W, user_num,
                       item_num, users, items, C, (int)topk, scores, out_ids);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // extern "C"
