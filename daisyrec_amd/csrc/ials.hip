// iALS / WRMF (Hu, Koren, Volinsky 2008): the Gram matrix of an fp32 factor table in fp64, one half-sweep
// of alternating least squares - per CSR row the normal equations A x = b accumulated on the fp64 MFMA, a Cholesky
// factorisation and the two triangular solves in LDS - and the objective by the Gram trick.  No kernel here waits on
// another workgroup, uses a floating-point atomic, or loops on a data-dependent condition without a bound; every sum runs
// in a fixed order, so two runs give the same bits whatever workgroup takes which row.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace daisy {
namespace {

typedef double doublex4 __attribute__((ext_vector_type(4)));

constexpr int kIalsMaxD = DAISY_IALS_MAX_D;
constexpr int kIalsGramRows = 256;          // default rows per block of the Gram pass ...
constexpr int kIalsGramMaxBlocks = 256;     // ... grown so that there are at most this many partial products
constexpr int kIalsGramMaxY = 16;           // workgroups that share one row block's tiles
constexpr int kIalsBatch = 16;              // row entries staged in LDS at a time: four MFMA steps of four entries
constexpr int kIalsWaves = kBlock / kWave;
constexpr int kIalsMaxGrid = 1 << 22;       // rows beyond that many workgroups are taken in a grid-stride loop
constexpr int kObjBlock = 1024;             // the single workgroup that adds the rows' partial objectives

// ---- Gram ----------------------------------------------------------------------------------------------------------------
// k_psvd_gram_partial's scheme on an fp32 table with a row pitch: tile (ti, tj), ti <= tj, of one row block's Y^T Y per
// wave at a time.  v_mfma_f64_16x16x4_f64: lane l feeds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] and gets
// D[row = (l >> 4) + 4 reg][col = l & 15], reg 0..3.
__global__ __launch_bounds__(kBlock) void k_ials_gram_partial(const float *__restrict__ Y, int64_t n, int64_t ld, int d,
                                                              int64_t block_rows, double *__restrict__ P) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int ct = (d + 15) / 16;
    const int ntiles = ct * (ct + 1) / 2;
    const int64_t r0 = (int64_t)blockIdx.x * block_rows;
    const int64_t r1 = (r0 + block_rows < n) ? r0 + block_rows : n;
    double *__restrict__ Pb = P + (int64_t)blockIdx.x * d * d;
    for (int t = blockIdx.y * kIalsWaves + wave; t < ntiles; t += gridDim.y * kIalsWaves) {
        int ti = 0, rem = t;
        while (rem >= ct - ti) { rem -= ct - ti; ++ti; }         // (at most ct steps)
        const int tj = ti + rem;
        const int ca = ti * 16 + (lane & 15), cb = tj * 16 + (lane & 15);
        const bool va = ca < d, vb = cb < d;
        doublex4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int64_t k0 = r0; k0 < r1; k0 += 4) {
            const int64_t k = k0 + (lane >> 4);
            const bool vk = k < r1;
            const double a = (vk && va) ? (double)Y[k * ld + ca] : 0.0;
            const double b = (vk && vb) ? (double)Y[k * ld + cb] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = ti * 16 + (lane >> 4) + 4 * reg, cg = tj * 16 + (lane & 15);
            if (row < d && cg < d) Pb[(int64_t)row * d + cg] = acc[reg];
        }
    }
}

// G = the blocks' partial products added in block order; the tiles below the diagonal are the mirrored ones above
__global__ __launch_bounds__(kBlock) void k_ials_gram_reduce(const double *__restrict__ P, int64_t nblocks, int d,
                                                             double *__restrict__ G) {
    const int dd = d * d;
    for (int e = blockIdx.x * kBlock + threadIdx.x; e < dd; e += gridDim.x * kBlock) {
        const int i = e / d, j = e % d;
        const int src = (i / 16 <= j / 16) ? e : j * d + i;
        double s = 0.0;
        for (int64_t b = 0; b < nblocks; ++b) s += P[b * dd + src];
        G[e] = s;
    }
}

inline int64_t ials_gram_block_rows(int64_t n) {
    int64_t r = kIalsGramRows;
    const int64_t spread = (n + kIalsGramMaxBlocks - 1) / kIalsGramMaxBlocks;
    if (spread > r) r = spread;
    return (r + 3) / 4 * 4;
}

// ---- half-sweep ----------------------------------------------------------------------------------------------------------
// The LDS of one workgroup (doubles): a region that first stages the row's entries (two buffers of kIalsBatch table rows
// in fp32, DP = 16 T columns each) and then holds the system - the lower triangle of A packed by rows, row i at
// i (i + 1) / 2, with b as row d of it, so that the factorisation carries the forward solve along - followed by the two
// buffers' weights, the factor's diagonal and the row's entry window.
__host__ __device__ inline int ials_tri(int i) { return i * (i + 1) / 2; }
__host__ __device__ inline int ials_region_doubles(int d, int dp) {
    const int stage = 2 * kIalsBatch * dp / 2;                   // floats, two to a double
    const int sys = ials_tri(d + 1) + d + 1;
    return stage > sys ? stage : sys;
}
inline size_t ials_lds_bytes(int d) {
    const int dp = (d + 15) / 16 * 16;
    return (size_t)(ials_region_doubles(d, dp) + 4 * kIalsBatch + kIalsMaxD) * sizeof(double);
}

template <int T>
struct IalsTiles {
    static constexpr int N = T * (T + 1) / 2;                         // tiles of the lower triangle
    static constexpr int PER_WAVE = (N + kIalsWaves - 1) / kIalsWaves;  // tile wave + 4 m belongs to wave `wave`
};

struct IalsArgs {
    const int64_t *row_ptr;
    const int32_t *col;
    const float *val;
    int64_t rows, nnz, n_other;
    const float *Y;
    int64_t ldy;
    int d;
    const double *G;
    double alpha, reg;
    float *X;
    int64_t ldx;
    unsigned int *info;          // 0xFFFFFFFF, or 1 + the smallest row whose factorisation met a bad pivot
    double *dump_A, *dump_b;
};

// One workgroup per row at a time.  Accumulation: the row's entries in stored order, kIalsBatch at a time through LDS
// (the next batch's loads are in flight under this batch's products); a wave owns the 16 x 16 tiles wave, wave + 4, ...
// of the lower triangle and feeds each with A[i][k] = w_k y_k[16 ti + i], B[k][j] = y_k[16 tj + j] for four entries k per
// instruction, w = alpha r.  b: thread f adds (1 + w_k) y_k[f] in the same order.  Entries past the row's end are zeros
// (they add +0 exactly); a column id outside [0, n_other) contributes nothing.
template <int T>
__global__ __launch_bounds__(kBlock) void k_ials_half_sweep(const IalsArgs a) {
    extern __shared__ __attribute__((aligned(16))) double ials_lds[];
    constexpr int DP = 16 * T;
    constexpr int PER_THREAD = kIalsBatch * DP / kBlock;             // staged floats per thread and batch (= T)
    constexpr int NT = IalsTiles<T>::N, PW = IalsTiles<T>::PER_WAVE;
    const int d = a.d;
    const int region = ials_region_doubles(d, DP);
    float *s_y = reinterpret_cast<float *>(ials_lds);                // [2][kIalsBatch][DP]
    double *s_a = ials_lds;                                          // packed lower triangle, row d = b
    double *s_w = ials_lds + region;                                 // [2][kIalsBatch] alpha r
    double *s_c = s_w + 2 * kIalsBatch;                              // [2][kIalsBatch] 1 + alpha r
    double *s_l = s_c + 2 * kIalsBatch;                              // [d] the factor's diagonal
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const int quad = lane >> 4, col16 = lane & 15;

    int off_a[PW], off_b[PW];                                        // column offsets of this wave's tiles
#pragma unroll
    for (int m = 0; m < PW; ++m) {
        int t = wave + kIalsWaves * m;
        if (t >= NT) t = 0;
        int ti = 0;
        while (ials_tri(ti + 1) <= t) ++ti;                          // (at most T steps)
        off_a[m] = 16 * ti + col16;
        off_b[m] = 16 * (t - ials_tri(ti)) + col16;
    }

    for (int64_t row = blockIdx.x; row < a.rows; row += gridDim.x) {
        int64_t beg = a.row_ptr[row], end = a.row_ptr[row + 1];
        beg = beg < 0 ? 0 : (beg > a.nnz ? a.nnz : beg);
        end = end < beg ? beg : (end > a.nnz ? a.nnz : end);
        float *__restrict__ xrow = a.X + row * a.ldx;
        const bool dump = a.dump_A != nullptr || a.dump_b != nullptr;
        if (beg == end && !dump) {                                   // an empty row: exact zeros, nothing to factor
            if (tid < d) xrow[tid] = 0.f;
            continue;
        }
        __syncthreads();                                             // the previous row's system is no longer read

        doublex4 acc[PW];
#pragma unroll
        for (int m = 0; m < PW; ++m) acc[m] = doublex4{0.0, 0.0, 0.0, 0.0};
        double bacc = 0.0;
        float stage[PER_THREAD];
        double stage_w = 0.0;
        bool stage_ok = false;

        // element tid + kBlock p of a batch is column (tid % DP) of entry (tid / DP + (kBlock / DP) p)   [DP divides kBlock
        // or is a multiple of it: 16 T with T <= 8 ... not for T = 3, 5, 6, 7, hence the plain index arithmetic]
        auto fetch = [&](int64_t base) {
#pragma unroll
            for (int p = 0; p < PER_THREAD; ++p) {
                const int idx = tid + kBlock * p;
                const int r = idx / DP, f = idx % DP;
                const int64_t e = base + r;
                float v = 0.f;
                if (e < end && f < d) {
                    const int32_t c = a.col[e];
                    if (c >= 0 && c < a.n_other) v = a.Y[(int64_t)c * a.ldy + f];
                }
                stage[p] = v;
            }
            stage_ok = false;
            if (tid < kIalsBatch) {
                const int64_t e = base + tid;
                if (e < end) {
                    const int32_t c = a.col[e];
                    stage_ok = c >= 0 && c < a.n_other;
                    stage_w = a.alpha * (double)a.val[e];
                }
            }
        };
        auto commit = [&](int buf) {
#pragma unroll
            for (int p = 0; p < PER_THREAD; ++p) s_y[buf * kIalsBatch * DP + tid + kBlock * p] = stage[p];
            if (tid < kIalsBatch) {
                s_w[buf * kIalsBatch + tid] = stage_ok ? stage_w : 0.0;
                s_c[buf * kIalsBatch + tid] = stage_ok ? 1.0 + stage_w : 0.0;
            }
        };

        if (beg < end) {
            fetch(beg);
            commit(0);
        }
        __syncthreads();
        int buf = 0;
        for (int64_t base = beg; base < end; base += kIalsBatch, buf ^= 1) {
            const bool more = base + kIalsBatch < end;
            if (more) fetch(base + kIalsBatch);
            const int64_t left = end - base;
            const int live = left < kIalsBatch ? (int)left : kIalsBatch;
            const float *__restrict__ yb = s_y + buf * kIalsBatch * DP;
            const double *__restrict__ wb = s_w + buf * kIalsBatch;
#pragma unroll 1
            for (int k0 = 0; k0 < live; k0 += 4) {
                const int k = k0 + quad;
                const double w = wb[k];
#pragma unroll
                for (int m = 0; m < PW; ++m) {
                    if (wave + kIalsWaves * m < NT) {
                        const double ya = (double)yb[k * DP + off_a[m]], yc = (double)yb[k * DP + off_b[m]];
                        acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(w * ya, yc, acc[m], 0, 0, 0);
                    }
                }
            }
            if (tid < DP) {
                const double *__restrict__ cb = s_c + buf * kIalsBatch;
                for (int k = 0; k < live; ++k) bacc = fma(cb[k], (double)yb[k * DP + tid], bacc);
            }
            if (more) commit(buf ^ 1);
            __syncthreads();
        }

        // the system into LDS (the staging buffers are dead: the loop ended on a barrier): the sums, then + (G + reg I)
#pragma unroll
        for (int m = 0; m < PW; ++m) {
            const int t = wave + kIalsWaves * m;
            if (t < NT) {
                const int c = off_b[m];
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int r = off_a[m] - col16 + quad + 4 * reg;
                    if (r < d && c <= r) s_a[ials_tri(r) + c] = acc[m][reg];
                }
            }
        }
        if (tid < d) s_a[ials_tri(d) + tid] = bacc;
        __syncthreads();
        // (a pass of its own: with G's loads among the accumulators' stores the compiler held all of them in registers at
        // once - 148 VGPRs at d = 64 against 108 this way)
#pragma unroll 2
        for (int e = tid; e < d * d; e += kBlock) {
            const int r = e / d, c = e - r * d;
            if (c <= r) s_a[ials_tri(r) + c] += a.G[e] + (r == c ? a.reg : 0.0);
        }
        __syncthreads();
        if (dump) {
            if (a.dump_A) {
                double *__restrict__ da = a.dump_A + row * (int64_t)d * d;
                for (int e = tid; e < d * d; e += kBlock) {
                    const int i = e / d, j = e % d;
                    da[e] = i >= j ? s_a[ials_tri(i) + j] : s_a[ials_tri(j) + i];
                }
            }
            if (a.dump_b && tid < d) a.dump_b[row * (int64_t)d + tid] = s_a[ials_tri(d) + tid];
            if (beg == end) {                                        // (uniform) the empty row again
                if (tid < d) xrow[tid] = 0.f;
                continue;
            }
            __syncthreads();
        }

        // right-looking Cholesky on rows 0 .. d (row d is b: it leaves as z = L^-1 b).  Column j: l_jj = sqrt(pivot), the
        // column below it divided by l_jj, then A[i][c] -= A[i][j] A[c][j] for j < c <= i - an element's sum runs over j
        // ascending.  The pivot stays where it is; the diagonal of L goes to s_l.
        bool bad = false;
        const int ty = tid >> 4, tx = tid & 15;
        for (int j = 0; j < d; ++j) {
            const double piv = s_a[ials_tri(j) + j];
            if (!(piv > 0.0) || !(piv < INFINITY)) { bad = true; break; }          // (uniform: everyone read the same word)
            const double ljj = sqrt(piv);
            for (int i = j + 1 + tid; i <= d; i += kBlock) s_a[ials_tri(i) + j] /= ljj;
            if (tid == 0) s_l[j] = ljj;
            __syncthreads();
            for (int i = j + 1 + ty; i <= d; i += kBlock / 16) {
                const double lij = s_a[ials_tri(i) + j];
                const int chi = i < d ? i : d - 1;
                for (int c = j + 1 + tx; c <= chi; c += 16) s_a[ials_tri(i) + c] -= lij * s_a[ials_tri(c) + j];
            }
            __syncthreads();
        }
        if (bad) {
            if (tid < d) xrow[tid] = __builtin_nanf("");
            if (tid == 0) atomicMin(a.info, (unsigned int)(row < INT_MAX - 1 ? row + 1 : INT_MAX));
            continue;
        }
        // L^T x = z from the bottom up: x_i = z_i / l_ii, then z_j -= L[i][j] x_i for j < i (row i of L is contiguous)
        double *__restrict__ z = s_a + ials_tri(d);
        double mine = 0.0;
        for (int i = d - 1; i >= 0; --i) {
            const double xi = z[i] / s_l[i];
            if (tid == i) mine = xi;
            for (int j = tid; j < i; j += kBlock) z[j] -= s_a[ials_tri(i) + j] * xi;
            __syncthreads();
        }
        if (tid < d) xrow[tid] = (float)mine;
    }
}

__global__ void k_ials_info_final(unsigned int *info) {
    if (*info == 0xFFFFFFFFu) *info = 0u;
}

// ---- objective -----------------------------------------------------------------------------------------------------------
// One wave per row: partial[row] = x^T G x + reg |x|^2 + sum over the row's entries of (1 + alpha r)(1 - s)^2 - s^2,
// s = <x, y_i> in fp64.  x^T G x: lane j holds t_j = sum_k G[k][j] x_k (k ascending; G is symmetric, so the read is
// coalesced); the entries four at a time, sixteen lanes to a dot product (DPP adds), each quarter's terms in stored order;
// the wave's sums by the xor butterfly.  Fixed order throughout.
__global__ __launch_bounds__(kBlock) void k_ials_obj_rows(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                          const float *__restrict__ val, int64_t rows, int64_t nnz,
                                                          int64_t n_other, const float *__restrict__ X, int64_t ldx,
                                                          const float *__restrict__ Y, int64_t ldy, int d,
                                                          const double *__restrict__ G, double alpha, double reg,
                                                          double *__restrict__ partial) {
    __shared__ double s_x[kIalsWaves][kIalsMaxD];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int quad = lane >> 4, ql = lane & 15;
    for (int64_t base = (int64_t)blockIdx.x * kIalsWaves; base < rows; base += (int64_t)gridDim.x * kIalsWaves) {
        const int64_t row = base + wave;
        const bool valid = row < rows;
        __syncthreads();
        for (int f = lane; f < kIalsMaxD; f += kWave) s_x[wave][f] = (valid && f < d) ? (double)X[row * ldx + f] : 0.0;
        __syncthreads();
        if (!valid) continue;                                        // (the barriers above sit before this)
        const double *__restrict__ x = s_x[wave];
        double q = 0.0, xx = 0.0;
        for (int j = lane; j < d; j += kWave) {
            double t = 0.0;
            for (int k = 0; k < d; ++k) t = fma(G[k * d + j], x[k], t);
            q = fma(x[j], t, q);
            xx = fma(x[j], x[j], xx);
        }
        int64_t beg = row_ptr[row], end = row_ptr[row + 1];
        beg = beg < 0 ? 0 : (beg > nnz ? nnz : beg);
        end = end < beg ? beg : (end > nnz ? nnz : end);
        double terms = 0.0;
        for (int64_t e0 = beg; e0 < end; e0 += 4) {
            const int64_t e = e0 + quad;
            int32_t c = -1;
            float r = 0.f;
            if (e < end) { c = col[e]; r = val[e]; }
            const bool live = c >= 0 && c < n_other;
            const float *__restrict__ y = Y + (int64_t)(live ? c : 0) * ldy;
            double s = 0.0;
            for (int f = ql; f < d; f += 16) s = fma(x[f], (double)y[f], s);
            s += dpp_f64<kDppQuadXor1>(s);
            s += dpp_f64<kDppQuadXor2>(s);
            s += dpp_f64<kDppHalfMirror>(s);
            s += dpp_f64<kDppMirror>(s);
            if (live && ql == 0) {
                const double cw = 1.0 + alpha * (double)r, m = 1.0 - s;
                terms += cw * (m * m) - s * s;
            }
        }
        const double total = wave_sum_f64(q) + reg * wave_sum_f64(xx) + wave_sum_f64(terms);
        if (lane == 0) partial[row] = total;
    }
}

// out = the partials added in a fixed order (thread t: t, t + 1024, ...; then a tree) + reg trace(G)   [|Y|^2 = trace(Y^T Y)]
__global__ __launch_bounds__(kObjBlock) void k_ials_obj_reduce(const double *__restrict__ partial, int64_t rows,
                                                               const double *__restrict__ G, int d, double reg,
                                                               double *__restrict__ out) {
    __shared__ double s_sum[kObjBlock];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int64_t e = tid; e < rows; e += kObjBlock) s += partial[e];
    s_sum[tid] = s;
    __syncthreads();
    for (int half = kObjBlock / 2; half > 0; half >>= 1) {
        if (tid < half) s_sum[tid] += s_sum[tid + half];
        __syncthreads();
    }
    if (tid == 0) {
        double tr = 0.0;
        for (int k = 0; k < d; ++k) tr += G[k * d + k];
        *out = s_sum[0] + reg * tr;
    }
}

template <int T>
int launch_half_sweep(const IalsArgs &a, hipStream_t s) {
    const size_t lds = ials_lds_bytes(a.d);
    DAISY_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_ials_half_sweep<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)ials_lds_bytes(16 * T)));
    hipLaunchKernelGGL(k_ials_half_sweep<T>, dim3(grid_for(a.rows, 1, kIalsMaxGrid)), dim3(kBlock), lds, s, a);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

inline bool ials_finite(double x) { return x == x && x - x == 0.0; }

}  // namespace
}  // namespace daisy

using namespace daisy;

extern "C" {

size_t daisy_ials_gram_workspace_bytes(int64_t n, int32_t d) {
    if (n < 1 || d < 1 || d > kIalsMaxD) return 0;
    const int64_t rows = ials_gram_block_rows(n);
    const int64_t nblocks = (n + rows - 1) / rows;
    return align_up((size_t)nblocks * (size_t)d * (size_t)d * sizeof(double));
}

int daisy_ials_gram(const float *Y, int64_t n, int64_t ld, int32_t d, double *G, void *workspace, size_t workspace_bytes,
                    daisy_stream_t stream) {
    DAISY_CHECK_ARG(Y && G && workspace, "ials_gram: NULL argument");
    DAISY_CHECK_ARG(d >= 1 && d <= kIalsMaxD, "ials_gram: d=%d outside [1, %d]", d, kIalsMaxD);
    DAISY_CHECK_ARG(n >= 1, "ials_gram: n=%lld must be >= 1", (long long)n);
    DAISY_CHECK_ARG(ld >= d, "ials_gram: ld=%lld is below d=%d", (long long)ld, d);
    const size_t need = daisy_ials_gram_workspace_bytes(n, d);
    DAISY_CHECK_ARG(workspace_bytes >= need, "ials_gram: workspace of %zu bytes, need %zu (daisy_ials_gram_workspace_bytes)",
                    workspace_bytes, need);
    const int64_t rows = ials_gram_block_rows(n);
    const int64_t nblocks = (n + rows - 1) / rows;
    hipStream_t s = as_stream(stream);
    const int ct = (d + 15) / 16;
    const int ntiles = ct * (ct + 1) / 2;
    int gy = (ntiles + kIalsWaves - 1) / kIalsWaves;
    if (gy > kIalsGramMaxY) gy = kIalsGramMaxY;
    double *P = static_cast<double *>(workspace);
    hipLaunchKernelGGL(k_ials_gram_partial, dim3((unsigned)nblocks, (unsigned)gy), dim3(kBlock), 0, s, Y, n, ld, (int)d, rows, P);
    DAISY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ials_gram_reduce, dim3(grid_for((int64_t)d * d, kBlock)), dim3(kBlock), 0, s, P, nblocks, (int)d, G);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_ials_half_sweep(const int64_t *row_ptr, const int32_t *col, const float *val, int64_t rows, int64_t nnz,
                          int64_t n_other, const float *Y, int64_t ldy, int32_t d, const double *G, double alpha, double reg,
                          float *X, int64_t ldx, int32_t *info, double *dump_A, double *dump_b, daisy_stream_t stream) {
    DAISY_CHECK_ARG(row_ptr && col && val && Y && G && X && info, "ials_half_sweep: NULL argument");
    DAISY_CHECK_ARG(d >= 1 && d <= kIalsMaxD, "ials_half_sweep: d=%d outside [1, %d]", d, kIalsMaxD);
    DAISY_CHECK_ARG(rows >= 0 && nnz >= 0, "ials_half_sweep: rows=%lld nnz=%lld must be >= 0", (long long)rows, (long long)nnz);
    DAISY_CHECK_ARG(n_other >= 1 && n_other <= INT_MAX, "ials_half_sweep: n_other=%lld outside [1, 2^31)", (long long)n_other);
    DAISY_CHECK_ARG(ldy >= d && ldx >= d, "ials_half_sweep: ldy=%lld ldx=%lld below d=%d", (long long)ldy, (long long)ldx, d);
    DAISY_CHECK_ARG(ials_finite(alpha) && ials_finite(reg), "ials_half_sweep: alpha=%g reg=%g must be finite", alpha, reg);
    hipStream_t s = as_stream(stream);
    DAISY_HIP(hipMemsetAsync(info, 0xFF, sizeof(int32_t), s));
    if (rows > 0) {
        IalsArgs a;
        a.row_ptr = row_ptr; a.col = col; a.val = val; a.rows = rows; a.nnz = nnz; a.n_other = n_other;
        a.Y = Y; a.ldy = ldy; a.d = (int)d; a.G = G; a.alpha = alpha; a.reg = reg; a.X = X; a.ldx = ldx;
        a.info = reinterpret_cast<unsigned int *>(info); a.dump_A = dump_A; a.dump_b = dump_b;
        int rc = DAISY_OK;
        switch ((d + 15) / 16) {
            case 1: rc = launch_half_sweep<1>(a, s); break;
            case 2: rc = launch_half_sweep<2>(a, s); break;
            case 3: rc = launch_half_sweep<3>(a, s); break;
            case 4: rc = launch_half_sweep<4>(a, s); break;
            case 5: rc = launch_half_sweep<5>(a, s); break;
            case 6: rc = launch_half_sweep<6>(a, s); break;
            case 7: rc = launch_half_sweep<7>(a, s); break;
            default: rc = launch_half_sweep<8>(a, s); break;
        }
        if (rc != DAISY_OK) return rc;
    }
    hipLaunchKernelGGL(k_ials_info_final, dim3(1), dim3(1), 0, s, reinterpret_cast<unsigned int *>(info));
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

size_t daisy_ials_objective_workspace_bytes(int64_t rows) {
    if (rows < 0) return 0;
    return align_up((size_t)(rows > 0 ? rows : 1) * sizeof(double));
}

int daisy_ials_objective(const int64_t *row_ptr, const int32_t *col, const float *val, int64_t rows, int64_t nnz,
                         int64_t n_other, const float *X, int64_t ldx, const float *Y, int64_t ldy, int32_t d, const double *G,
                         double alpha, double reg, double *out, void *workspace, size_t workspace_bytes,
                         daisy_stream_t stream) {
    DAISY_CHECK_ARG(row_ptr && col && val && X && Y && G && out && workspace, "ials_objective: NULL argument");
    DAISY_CHECK_ARG(d >= 1 && d <= kIalsMaxD, "ials_objective: d=%d outside [1, %d]", d, kIalsMaxD);
    DAISY_CHECK_ARG(rows >= 0 && nnz >= 0, "ials_objective: rows=%lld nnz=%lld must be >= 0", (long long)rows, (long long)nnz);
    DAISY_CHECK_ARG(n_other >= 1 && n_other <= INT_MAX, "ials_objective: n_other=%lld outside [1, 2^31)", (long long)n_other);
    DAISY_CHECK_ARG(ldy >= d && ldx >= d, "ials_objective: ldy=%lld ldx=%lld below d=%d", (long long)ldy, (long long)ldx, d);
    DAISY_CHECK_ARG(ials_finite(alpha) && ials_finite(reg), "ials_objective: alpha=%g reg=%g must be finite", alpha, reg);
    const size_t need = daisy_ials_objective_workspace_bytes(rows);
    DAISY_CHECK_ARG(workspace_bytes >= need, "ials_objective: workspace of %zu bytes, need %zu (daisy_ials_objective_workspace_bytes)",
                    workspace_bytes, need);
    hipStream_t s = as_stream(stream);
    double *partial = static_cast<double *>(workspace);
    if (rows > 0) {
        hipLaunchKernelGGL(k_ials_obj_rows, dim3(grid_for(rows, kIalsWaves, kMaxGridSparse)), dim3(kBlock), 0, s, row_ptr, col, val,
                           rows, nnz, n_other, X, ldx, Y, ldy, (int)d, G, alpha, reg, partial);
        DAISY_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_ials_obj_reduce, dim3(1), dim3(kObjBlock), 0, s, partial, rows, G, (int)d, reg, out);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // extern "C"
