// PureSVD (daisy/model/PureSVDRecommender.py): the pieces of scikit-learn's randomized_svd in fp64 - the
// sparse x tall-skinny product, the Gram matrix and the tall-skinny x small product on the fp64 MFMA, a Cholesky
// factorisation that drops dependent columns (Cholesky-QR2 is two rounds of Gram, Cholesky, product), a one-sided Jacobi
// SVD of the small projected matrix, and scoring with a top-k taken on the fp64 keys.  No kernel here waits on another
// workgroup, uses a floating-point atomic, or loops on a data-dependent condition without a bound.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "score_f64.h"
#include "topk_f64.h"

namespace daisy {
namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int kPsvdMaxC = DAISY_PSVD_MAX_C;
constexpr int kPsvdGramRows = 256;          // default rows per block of the Gram pass ...
constexpr int kPsvdGramMaxBlocks = 256;     // ... grown so that there are at most this many partial products
constexpr int kPsvdGramMaxY = 16;           // workgroups that share one row block's tiles
constexpr int kJacobiBlock = 1024;          // the Jacobi workgroup: 16 waves, one pair of rows per wave at a time
constexpr int kJacobiWaves = kJacobiBlock / kWave;
constexpr double kEps = 2.220446049250313e-16;   // 2^-52

// ---- sparse x tall-skinny ----------------------------------------------------------------------------------------------
// one workgroup per row at a time, thread t owns column t: the row's non-zeros in stored order
__global__ __launch_bounds__(kBlock) void k_psvd_spmm(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                      const float *__restrict__ val, int64_t n_rows, int64_t n_cols,
                                                      const double *__restrict__ X, int c, double *__restrict__ Y) {
    const int t = threadIdx.x;
    if (t >= c) return;
    for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const int64_t beg = row_ptr[r], end = row_ptr[r + 1];
        double acc = 0.0;
        for (int64_t e = beg; e < end; ++e) {
            const int32_t j = col[e];
            if (j >= 0 && j < n_cols) acc = fma((double)val[e], X[(int64_t)j * c + t], acc);
        }
        Y[r * c + t] = acc;
    }
}

// ---- Gram --------------------------------------------------------------------------------------------------------------
// Tile (ti, tj), ti <= tj, of one row block's Y^T Y per wave at a time.  v_mfma_f64_16x16x4_f64: lane l feeds
// A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] and gets D[row = (l >> 4) + 4 reg][col = l & 15], reg 0..3.
// Here A[i][k] = Y[k][16 ti + i], B[k][j] = Y[k][16 tj + j]; rows past the block and columns past c are zeros in
// registers.
__global__ __launch_bounds__(kBlock) void k_psvd_gram_partial(const double *__restrict__ Y, int64_t n, int c,
                                                              int64_t block_rows, double *__restrict__ P) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int ct = (c + 15) / 16;
    const int ntiles = ct * (ct + 1) / 2;
    const int64_t r0 = (int64_t)blockIdx.x * block_rows;
    const int64_t r1 = (r0 + block_rows < n) ? r0 + block_rows : n;
    double *__restrict__ Pb = P + (int64_t)blockIdx.x * c * c;
    for (int t = blockIdx.y * (kBlock / kWave) + wave; t < ntiles; t += gridDim.y * (kBlock / kWave)) {
        int ti = 0, rem = t;
        while (rem >= ct - ti) { rem -= ct - ti; ++ti; }         // (at most ct steps)
        const int tj = ti + rem;
        const int ca = ti * 16 + (lane & 15), cb = tj * 16 + (lane & 15);
        const bool va = ca < c, vb = cb < c;
        doublex4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int64_t k0 = r0; k0 < r1; k0 += 4) {
            const int64_t k = k0 + (lane >> 4);
            const bool vk = k < r1;
            const double a = (vk && va) ? Y[k * c + ca] : 0.0;
            const double b = (vk && vb) ? Y[k * c + cb] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = ti * 16 + (lane >> 4) + 4 * reg, cg = tj * 16 + (lane & 15);
            if (row < c && cg < c) Pb[(int64_t)row * c + cg] = acc[reg];
        }
    }
}

// G = the blocks' partial products added in block order; the tiles below the diagonal are the mirrored ones above
__global__ __launch_bounds__(kBlock) void k_psvd_gram_reduce(const double *__restrict__ P, int64_t nblocks, int c,
                                                             double *__restrict__ G) {
    const int64_t cc = (int64_t)c * c;
    for (int64_t e = blockIdx.x * (int64_t)kBlock + threadIdx.x; e < cc; e += (int64_t)gridDim.x * kBlock) {
        const int i = (int)(e / c), j = (int)(e % c);
        const int64_t src = (i / 16 <= j / 16) ? e : (int64_t)j * c + i;
        double s = 0.0;
        for (int64_t b = 0; b < nblocks; ++b) s += P[b * cc + src];
        G[e] = s;
    }
}

// ---- tall-skinny x small -----------------------------------------------------------------------------------------------
// C[n, c2] = Y[n, c] T[c, c2]: one 16 x 16 tile of C per wave at a time, A[i][k] = Y[16 rt + i][k], B[k][j] = T[k][16 tj + j]
__global__ __launch_bounds__(kBlock) void k_psvd_gemm(const double *__restrict__ Y, const double *__restrict__ T,
                                                      double *__restrict__ Cm, int64_t n, int c, int c2) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int ct2 = (c2 + 15) / 16;
    const int64_t tiles = ((n + 15) / 16) * ct2;
    for (int64_t w = (int64_t)blockIdx.x * (kBlock / kWave) + wave; w < tiles; w += (int64_t)gridDim.x * (kBlock / kWave)) {
        const int64_t rt = w / ct2;
        const int tj = (int)(w % ct2);
        const int64_t row = rt * 16 + (lane & 15);
        const int cb = tj * 16 + (lane & 15);
        const bool vr = row < n, vc = cb < c2;
        doublex4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < c; k0 += 4) {
            const int k = k0 + (lane >> 4);
            const bool vk = k < c;
            const double a = (vr && vk) ? Y[row * c + k] : 0.0;
            const double b = (vk && vc) ? T[(int64_t)k * c2 + cb] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t r = rt * 16 + (lane >> 4) + 4 * reg;
            if (r < n && vc) Cm[r * c2 + cb] = acc[reg];
        }
    }
}

// ---- Cholesky with dropped columns ---------------------------------------------------------------------------------------
// One workgroup, thread k owns column k.  Row j of R needs the rows above it: left-looking, one barrier pair per row.
// Then thread k solves R_KK x = e_k (K: the kept columns) from the bottom up for column k of the inverse; it only reads
// what it wrote itself.
__global__ __launch_bounds__(kBlock) void k_psvd_chol(const double *__restrict__ G, int c, double thresh, double *R,
                                                      double *Rinv, int32_t *__restrict__ dropped) {
    __shared__ double s_d;
    __shared__ unsigned char s_keep[kPsvdMaxC];
    const int k = threadIdx.x;
    int ndrop = 0;
    for (int j = 0; j < c; ++j) {
        double s = 0.0;
        if (k >= j && k < c)
            for (int i = 0; i < j; ++i) s += R[i * c + j] * R[i * c + k];
        const double gjj = G[j * c + j];
        if (k == j) s_d = gjj - s;
        __syncthreads();
        const double d = s_d;
        const bool keep = d > thresh * gjj;                    // (false for a pivot that is not a number)
        if (k < c) {
            double v = 0.0;
            if (keep && k >= j) {
                const double rjj = sqrt(d);
                v = (k == j) ? rjj : (G[j * c + k] - s) / rjj;
            }
            R[j * c + k] = v;
        }
        if (k == 0) s_keep[j] = keep ? 1 : 0;
        ndrop += keep ? 0 : 1;
        __syncthreads();
    }
    if (k == 0) *dropped = ndrop;
    if (k >= c) return;
    const bool keep_k = s_keep[k] != 0;
    for (int i = c - 1; i >= 0; --i) {
        double x = 0.0;
        if (keep_k && i <= k && s_keep[i]) {
            if (i == k) {
                x = 1.0 / R[k * c + k];
            } else {
                double s = 0.0;
                for (int l = i + 1; l <= k; ++l) s += R[i * c + l] * Rinv[l * c + k];
                x = -s / R[i * c + i];
            }
        }
        Rinv[i * c + k] = x;
    }
}

// ---- one-sided Jacobi SVD ------------------------------------------------------------------------------------------------
// W = J A: the rotations J make W's rows orthogonal, so that W = diag(s) V^T and A = J^T diag(s) V^T.  Round-robin: in
// round r of a sweep the cc / 2 pairs are disjoint (cc: c rounded up to even; a pair with the dummy row is skipped), every
// wave takes pairs in turn and a barrier ends the round.  W and J live in the workspace (global memory: 2 x 512 KB at
// c = 256), a lane holds elements lane, lane + 64, ... of both rows of its wave's pair.
__global__ __launch_bounds__(kJacobiBlock) void k_psvd_jacobi(const double *__restrict__ A, int c, int max_sweeps, double *W,
                                                              double *Jt, double *__restrict__ U, double *__restrict__ S,
                                                              double *__restrict__ V, int32_t *__restrict__ info) {
    __shared__ int s_rot;
    __shared__ double s_norm[kPsvdMaxC];
    __shared__ int s_perm[kPsvdMaxC];
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    for (int e = tid; e < c * c; e += kJacobiBlock) {
        W[e] = A[e];
        Jt[e] = (e / c == e % c) ? 1.0 : 0.0;
    }
    if (tid == 0) s_rot = 0;
    __syncthreads();
    const double tol = sqrt((double)c) * kEps;
    const int cc = c + (c & 1);
    int status = DAISY_PSVD_NOT_CONVERGED, sweeps = 0;
    for (int sweep = 0; sweep < max_sweeps; ++sweep) {
        int rot = 0;
        for (int r = 0; r < cc - 1; ++r) {
            for (int pk = wave; pk < cc / 2; pk += kJacobiWaves) {
                const int a = (pk == 0) ? cc - 1 : (r + pk) % (cc - 1);
                const int b = (pk == 0) ? r : (r - pk + cc - 1) % (cc - 1);
                const int p = a < b ? a : b, q = a < b ? b : a;
                if (q >= c) continue;
                double *wp = W + p * c, *wq = W + q * c;
                double xp[4], xq[4];
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int e = lane + kWave * m;
                    xp[m] = e < c ? wp[e] : 0.0;
                    xq[m] = e < c ? wq[e] : 0.0;
                    alpha += xp[m] * xp[m];
                    beta += xq[m] * xq[m];
                    gamma += xp[m] * xq[m];
                }
                alpha = wave_sum_f64(alpha);
                beta = wave_sum_f64(beta);
                gamma = wave_sum_f64(gamma);
                if (!(fabs(gamma) > tol * sqrt(alpha) * sqrt(beta))) continue;        // (uniform over the wave)
                ++rot;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                double *jp = Jt + p * c, *jq = Jt + q * c;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int e = lane + kWave * m;
                    if (e < c) {
                        wp[e] = cs * xp[m] - sn * xq[m];
                        wq[e] = sn * xp[m] + cs * xq[m];
                        const double up = jp[e], uq = jq[e];
                        jp[e] = cs * up - sn * uq;
                        jq[e] = sn * up + cs * uq;
                    }
                }
            }
            __syncthreads();
        }
        if (lane == 0 && rot) atomicAdd(&s_rot, rot);
        __syncthreads();
        const int total = s_rot;
        __syncthreads();
        if (tid == 0) s_rot = 0;
        sweeps = sweep + 1;
        if (total == 0) { status = DAISY_PSVD_CONVERGED; break; }
    }
    // the rows' norms are the singular values; sorted non-increasing, ties in row order
    for (int i = wave; i < c; i += kJacobiWaves) {
        double x = 0.0;
        for (int e = lane; e < c; e += kWave) x += W[i * c + e] * W[i * c + e];
        x = wave_sum_f64(x);
        if (lane == 0) s_norm[i] = sqrt(x);
    }
    __syncthreads();
    if (tid < c) {
        const double mine = s_norm[tid];
        const bool mine_nan = mine != mine;       // (not-a-numbers go last, in row order: the ranks stay a permutation)
        int rank = 0;
        for (int j = 0; j < c; ++j) {
            const double o = s_norm[j];
            const bool o_nan = o != o;
            const bool before = mine_nan ? (!o_nan || j < tid) : (!o_nan && (o > mine || (o == mine && j < tid)));
            rank += before ? 1 : 0;
        }
        s_perm[rank] = tid;
    }
    __syncthreads();
    for (int e = tid; e < c * c; e += kJacobiBlock) {
        const int j = e / c, i = e % c;
        const int src = s_perm[i];
        const double sv = s_norm[src];
        U[e] = Jt[src * c + j];
        V[e] = sv > 0.0 ? W[src * c + j] / sv : 0.0;
    }
    if (tid < c) S[tid] = s_norm[s_perm[tid]];
    if (tid == 0) { info[0] = status; info[1] = sweeps; }
}

// ---- scores and top-k on the fp64 keys ------------------------------------------------------------------------------------
// One workgroup per user row: the row's scores (thread per candidate, factors in ascending order), then the top-k of
// topk_f64.h (score descending, position ascending).
__global__ __launch_bounds__(kBlock) void k_psvd_rank(const double *__restrict__ user_vec, const double *__restrict__ item_vec,
                                                      int64_t U, int64_t I, int k, const int64_t *__restrict__ users,
                                                      const int64_t *__restrict__ items, int64_t C, int topk,
                                                      double *scores, int64_t *__restrict__ out_ids) {
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t u = users[b];
    const bool valid = u >= 0 && u < U;
    const double *__restrict__ uv = user_vec + (valid ? u : 0) * k;
    double *row = scores + b * C;
    for (int64_t cidx = tid; cidx < C; cidx += kBlock) {
        const int64_t it = items ? items[b * C + cidx] : cidx;
        double s = 0.0;
        if (valid && it >= 0 && it < I) s = psvd_score(uv, item_vec + it * k, k);
        row[cidx] = s;
    }
    if (!out_ids) return;
    topk_f64_select(row, C, topk, items ? items + b * C : nullptr, out_ids + b * topk);
}

inline int64_t gram_block_rows(int64_t n, int64_t block_rows) {
    int64_t r = block_rows;
    if (r <= 0) {
        r = kPsvdGramRows;
        const int64_t spread = (n + kPsvdGramMaxBlocks - 1) / kPsvdGramMaxBlocks;
        if (spread > r) r = spread;
    }
    return (r + 3) / 4 * 4;
}

}  // namespace
}  // namespace daisy

using namespace daisy;

extern "C" {

int daisy_psvd_spmm(const int64_t *row_ptr, const int32_t *col, const float *val, int64_t n_rows, int64_t n_cols,
                    const double *X, int32_t c, double *Y, daisy_stream_t stream) {
    DAISY_CHECK_ARG(row_ptr && col && val && X && Y, "psvd_spmm: NULL argument");
    DAISY_CHECK_ARG(n_rows >= 0 && n_cols >= 1 && n_cols <= INT_MAX, "psvd_spmm: n_rows=%lld n_cols=%lld", (long long)n_rows,
                    (long long)n_cols);
    DAISY_CHECK_ARG(c >= 1 && c <= kPsvdMaxC, "psvd_spmm: c=%d outside [1, %d]", c, kPsvdMaxC);
    if (n_rows == 0) return DAISY_OK;
    hipLaunchKernelGGL(k_psvd_spmm, dim3(grid_for(n_rows, 1, kMaxGridSparse)), dim3(kBlock), 0, as_stream(stream), row_ptr, col,
                       val, n_rows, n_cols, X, (int)c, Y);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int64_t daisy_psvd_gram_block_rows(int64_t n, int64_t block_rows) {
    if (n < 1) return 0;
    return gram_block_rows(n, block_rows);
}

size_t daisy_psvd_gram_workspace_bytes(int64_t n, int32_t c, int64_t block_rows) {
    if (n < 1 || c < 1 || c > kPsvdMaxC) return 0;
    const int64_t rows = gram_block_rows(n, block_rows);
    const int64_t nblocks = (n + rows - 1) / rows;
    return align_up((size_t)nblocks * (size_t)c * (size_t)c * sizeof(double));
}

int daisy_psvd_gram(const double *Y, int64_t n, int32_t c, double *G, int64_t block_rows, void *workspace,
                    size_t workspace_bytes, daisy_stream_t stream) {
    DAISY_CHECK_ARG(Y && G && workspace, "psvd_gram: NULL argument");
    DAISY_CHECK_ARG(n >= 1, "psvd_gram: n=%lld must be >= 1", (long long)n);
    DAISY_CHECK_ARG(c >= 1 && c <= kPsvdMaxC, "psvd_gram: c=%d outside [1, %d]", c, kPsvdMaxC);
    const int64_t rows = gram_block_rows(n, block_rows);
    const int64_t nblocks = (n + rows - 1) / rows;
    DAISY_CHECK_ARG(nblocks <= 65535, "psvd_gram: block_rows=%lld makes %lld blocks (at most 65535)", (long long)block_rows,
                    (long long)nblocks);
    const size_t need = daisy_psvd_gram_workspace_bytes(n, c, block_rows);
    DAISY_CHECK_ARG(workspace_bytes >= need, "psvd_gram: workspace of %zu bytes, need %zu (daisy_psvd_gram_workspace_bytes)",
                    workspace_bytes, need);
    hipStream_t s = as_stream(stream);
    const int ct = (c + 15) / 16;
    const int ntiles = ct * (ct + 1) / 2;
    int gy = (ntiles + kBlock / kWave - 1) / (kBlock / kWave);
    if (gy > kPsvdGramMaxY) gy = kPsvdGramMaxY;
    double *P = static_cast<double *>(workspace);
    hipLaunchKernelGGL(k_psvd_gram_partial, dim3((unsigned)nblocks, (unsigned)gy), dim3(kBlock), 0, s, Y, n, (int)c, rows, P);
    DAISY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_psvd_gram_reduce, dim3(grid_for((int64_t)c * c, kBlock)), dim3(kBlock), 0, s, P, nblocks, (int)c, G);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_psvd_chol(const double *G, int32_t c, int64_t n, double *R, double *Rinv, int32_t *dropped,
                    daisy_stream_t stream) {
    DAISY_CHECK_ARG(G && R && Rinv && dropped, "psvd_chol: NULL argument");
    DAISY_CHECK_ARG(c >= 1 && c <= kPsvdMaxC, "psvd_chol: c=%d outside [1, %d]", c, kPsvdMaxC);
    DAISY_CHECK_ARG(n >= 1, "psvd_chol: n=%lld must be >= 1", (long long)n);
    hipLaunchKernelGGL(k_psvd_chol, dim3(1), dim3(kBlock), 0, as_stream(stream), G, (int)c, 64.0 * (double)n * kEps, R, Rinv,
                       dropped);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_psvd_gemm(const double *Y, const double *T, double *C, int64_t n, int32_t c, int32_t c2, daisy_stream_t stream) {
    DAISY_CHECK_ARG(Y && T && C, "psvd_gemm: NULL argument");
    DAISY_CHECK_ARG(n >= 0, "psvd_gemm: n=%lld must be >= 0", (long long)n);
    DAISY_CHECK_ARG(c >= 1 && c <= kPsvdMaxC && c2 >= 1 && c2 <= kPsvdMaxC, "psvd_gemm: c=%d c2=%d outside [1, %d]", c, c2,
                    kPsvdMaxC);
    if (n == 0) return DAISY_OK;
    const int64_t tiles = ((n + 15) / 16) * ((c2 + 15) / 16);
    hipLaunchKernelGGL(k_psvd_gemm, dim3(grid_for(tiles, kBlock / kWave, kMaxGridSparse)), dim3(kBlock), 0, as_stream(stream), Y,
                       T, C, n, (int)c, (int)c2);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

size_t daisy_psvd_jacobi_workspace_bytes(int32_t c) {
    if (c < 1 || c > kPsvdMaxC) return 0;
    return 2 * align_up((size_t)c * (size_t)c * sizeof(double));
}

int daisy_psvd_jacobi(const double *A, int32_t c, int32_t max_sweeps, double *U, double *s, double *V, int32_t *info,
                      void *workspace, size_t workspace_bytes, daisy_stream_t stream) {
    DAISY_CHECK_ARG(A && U && s && V && info && workspace, "psvd_jacobi: NULL argument");
    DAISY_CHECK_ARG(c >= 1 && c <= kPsvdMaxC, "psvd_jacobi: c=%d outside [1, %d]", c, kPsvdMaxC);
    DAISY_CHECK_ARG(max_sweeps >= 1 && max_sweeps <= 1000, "psvd_jacobi: max_sweeps=%d outside [1, 1000]", max_sweeps);
    const size_t need = daisy_psvd_jacobi_workspace_bytes(c);
    DAISY_CHECK_ARG(workspace_bytes >= need, "psvd_jacobi: workspace of %zu bytes, need %zu (daisy_psvd_jacobi_workspace_bytes)",
                    workspace_bytes, need);
    double *W = static_cast<double *>(workspace);
    double *Jt = reinterpret_cast<double *>(static_cast<char *>(workspace) + need / 2);
    hipLaunchKernelGGL(k_psvd_jacobi, dim3(1), dim3(kJacobiBlock), 0, as_stream(stream), A, (int)c, (int)max_sweeps, W, Jt, U, s,
                       V, info);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_psvd_rank(const double *user_vec, const double *item_vec, int64_t user_num, int64_t item_num, int32_t k,
                    const int64_t *users, int64_t B, const int64_t *items, int64_t C, int32_t topk, double *scores,
                    int64_t *out_ids, daisy_stream_t stream) {
    DAISY_CHECK_ARG(user_vec && item_vec && scores, "psvd_rank: NULL argument");
    DAISY_CHECK_ARG(user_num >= 1 && item_num >= 1, "psvd_rank: user_num=%lld item_num=%lld", (long long)user_num,
                    (long long)item_num);
    DAISY_CHECK_ARG(k >= 1 && k <= kPsvdMaxC, "psvd_rank: k=%d factors outside [1, %d]", k, kPsvdMaxC);
    DAISY_CHECK_ARG(B >= 0 && B <= INT_MAX && (B == 0 || users), "psvd_rank: B=%lld users (NULL users?)", (long long)B);
    DAISY_CHECK_ARG(items ? C >= 1 : C == item_num, "psvd_rank: C=%lld candidates per user (item_num when items == NULL)",
                    (long long)C);
    DAISY_CHECK_ARG(!out_ids || (topk >= 1 && topk <= C), "psvd_rank: topk=%d outside [1, C=%lld]", topk, (long long)C);
    if (B == 0) return DAISY_OK;
    hipLaunchKernelGGL(k_psvd_rank, dim3((unsigned)B), dim3(kBlock), 0, as_stream(stream), user_vec, item_vec, user_num, item_num,
                       (int)k, users, items, C, (int)topk, scores, out_ids);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // extern "C"
