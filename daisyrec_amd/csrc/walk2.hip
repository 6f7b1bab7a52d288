// Two-hop walk with a per-row top-K (RP3beta / P3alpha): for every row i of a sparse A the K largest
// strictly positive entries of row i of (A B) diag(col_scale), A and B both CSR - the dense product is never formed.
// One workgroup owns one source row at a time (rows are handed out by an integer counter) and a dense fp32 accumulator
// over the n_cols columns, in LDS or in a slab of the caller's workspace.  No floating-point atomics: column j belongs to
// wave (j / 32) mod 4, every wave walks the row's entries u in stored order and adds the entries of B's row u that it owns, so
// acc[j] receives its terms in ascending u whatever the grid, the path or the hand-out of rows.
#include <limits.h>

#include "common.h"

namespace daisy {
namespace {

constexpr int kW2Waves = kBlock / kWave;
constexpr int kW2OwnShift = 5;                       // columns are owned in runs of 32: wave (j / 32) mod 4
constexpr int kW2Ahead = 4;                         // 64-entry steps of a row of B loaded before they are used
constexpr int kW2CUs = 256;
constexpr size_t kW2LdsPerCU = 160 * 1024;
constexpr size_t kW2StaticLds = 13 * 1024;          // the histograms and the kept pairs, rounded up
constexpr int kW2MaxGroups = 65536;
constexpr size_t kW2CounterBytes = 256;

inline bool walk2_lds(int32_t path, int64_t n_cols) {
    return path == DAISY_SLIM_PATH_LDS || (path == DAISY_SLIM_PATH_AUTO && n_cols <= DAISY_WALK2_LDS_COLS);
}
inline size_t walk2_slab_bytes(int64_t n_cols) { return align_up((size_t)n_cols * sizeof(float)); }
// the workgroups of a launch: the caller's count, or as many as fit the CUs at once (LDS) / 2 per CU (global slabs)
inline int walk2_groups(int64_t n_rows, int64_t n_cols, bool lds, int32_t n_groups) {
    int64_t g = n_groups;
    if (g <= 0) {
        size_t per_cu = lds ? kW2LdsPerCU / ((size_t)n_cols * sizeof(float) + kW2StaticLds) : 2;
        per_cu = per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu);
        g = (int64_t)kW2CUs * (int64_t)per_cu;
    }
    if (g > n_rows) g = n_rows;
    return (int)(g < 1 ? 1 : g);
}

// Every product and every sum is rounded on its own: nothing below is contracted into a fused multiply-add.  Plain
// operators, as in knn_weight: __fmul_rn / __fadd_rn are inline functions of a header compiled with contraction allowed,
// and a product and a sum that both carry that licence are fused again after inlining.
#pragma clang fp contract(off)

// larger weight <=> larger key among the strictly positive weights; zero, negative and NaN share the key 0: never kept
__device__ __forceinline__ uint32_t walk2_key(float w) { return w > 0.f ? __float_as_uint(w) : 0u; }

__device__ __forceinline__ float walk2_weight(const float *acc, const float *__restrict__ col_scale, int64_t j, int64_t diag) {
    float w = acc[j];
    if (col_scale) w = w * col_scale[j];
    return j == diag ? 0.f : w;
}

template <bool LDS>
__device__ __forceinline__ void walk2_add(float *acc, int32_t j, float a, float b, int64_t n_cols, int wave) {
    if (j >= 0 && j < n_cols && ((j >> kW2OwnShift) & (kW2Waves - 1)) == wave) {
        const float p = a * b;          // rounded on its own (contraction is off from the pragma on)
        acc[j] = acc[j] + p;
    }
}

// kW2Ahead steps of 64 entries of one row of B, in registers: all their loads are in flight before the first is used
struct Walk2Ahead {
    int32_t j[kW2Ahead];
    float v[kW2Ahead];
    __device__ __forceinline__ void load(const int32_t *__restrict__ b_col, const float *__restrict__ b_val, long long beg,
                                         long long end, int lane) {
#pragma unroll
        for (int c = 0; c < kW2Ahead; ++c) {
            const long long t = beg + c * kWave + lane;
            j[c] = -1;                                          // past the row's end: walk2_add skips it
            v[c] = 0.f;
            if (t < end) { j[c] = b_col[t]; v[c] = b_val[t]; }
        }
    }
    template <bool LDS>
    __device__ __forceinline__ void add(float *acc, float a, int64_t n_cols, int wave) const {
#pragma unroll
        for (int c = 0; c < kW2Ahead; ++c) walk2_add<LDS>(acc, j[c], a, v[c], n_cols, wave);
    }
};

// The read-modify-writes of one wave on its own columns need no barrier between two users: DS operations of a wave
// execute in order (LDS); the global slab takes a workgroup-scope fence, which waits for the wave's stores.
template <bool LDS>
__device__ __forceinline__ void walk2_user_done() {
    if (LDS)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    else
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
}

template <bool LDS>
__global__ __launch_bounds__(kBlock) void k_walk2_topk(const int64_t *__restrict__ a_ptr, const int32_t *__restrict__ a_col,
                                                       const float *__restrict__ a_val, int64_t n_rows, int64_t inner,
                                                       const int64_t *__restrict__ b_ptr, const int32_t *__restrict__ b_col,
                                                       const float *__restrict__ b_val, int64_t n_cols,
                                                       const float *__restrict__ col_scale, int zero_diagonal, int normalize,
                                                       int K, int32_t *__restrict__ count, int32_t *__restrict__ cols,
                                                       float *__restrict__ vals, unsigned long long *next_row, float *slabs,
                                                       size_t slab_pitch) {
    extern __shared__ __attribute__((aligned(16))) float w2_lds[];
    __shared__ __attribute__((aligned(16))) int s_hist[4][256];
    __shared__ int s_cnt[2][kW2Waves][2];
    __shared__ int32_t s_col[DAISY_KNN_MAX_K];
    __shared__ float s_val[DAISY_KNN_MAX_K];
    __shared__ long long s_row;
    __shared__ float s_sum;
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int keff = (int64_t)K < n_cols ? K : (int)n_cols;
    float *acc = LDS ? w2_lds : slabs + (size_t)blockIdx.x * slab_pitch;

    for (int64_t j = tid; j < n_cols; j += kBlock) acc[j] = 0.f;

    for (;;) {
        if (tid == 0) s_row = (long long)atomicAdd(next_row, 1ull);
        for (int e = tid; e < 4 * 256; e += kBlock) (&s_hist[0][0])[e] = 0;
        __syncthreads();                                   // the row, the cleared histograms and the cleared accumulator
        const int64_t i = s_row;
        if (i >= n_rows) break;

        // ---- accumulate: 64 entries of A's row at a time, one per lane; their users one after the other --------------
        const int64_t abeg = a_ptr[i], aend = a_ptr[i + 1];
        for (int64_t e0 = abeg; e0 < aend; e0 += kWave) {
            const int64_t e = e0 + lane;
            float a = 0.f;
            long long bb = 0, be = 0;
            if (e < aend) {
                const int32_t u = a_col[e];
                a = a_val[e];
                if (u >= 0 && u < inner) { bb = b_ptr[u]; be = b_ptr[u + 1]; }
            }
            const int cnt = aend - e0 < kWave ? (int)(aend - e0) : kWave;
            // the first 256 entries of the next user's row are loaded while this user's are added
            long long nb = __shfl(bb, 0, kWave), ne = __shfl(be, 0, kWave);
            Walk2Ahead nxt;
            nxt.load(b_col, b_val, nb, ne, lane);
#pragma unroll 1
            for (int k = 0; k < cnt; ++k) {
                const long long cb = nb, ce = ne;
                const Walk2Ahead cur = nxt;
                const float ak = __shfl(a, k, kWave);
                if (k + 1 < cnt) {
                    nb = __shfl(bb, k + 1, kWave);
                    ne = __shfl(be, k + 1, kWave);
                    nxt.load(b_col, b_val, nb, ne, lane);
                }
                cur.add<LDS>(acc, ak, n_cols, wave);
                for (long long t = cb + kW2Ahead * kWave; t < ce; t += kW2Ahead * kWave) {      // a longer row: 256 at a time
                    Walk2Ahead more;
                    more.load(b_col, b_val, t, ce, lane);
                    more.add<LDS>(acc, ak, n_cols, wave);
                }
                walk2_user_done<LDS>();
            }
        }
        __syncthreads();

        // ---- select: the key of the keff-th largest weight by four 8-bit histogram passes ---------------------------
        const int64_t diag = zero_diagonal ? i : -1;
        uint32_t prefix = 0u;
        int krem = keff;
#pragma unroll 1
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            const uint32_t hi_mask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
            int *hist = s_hist[pass];
            for (int64_t base = 0; base < n_cols; base += kBlock) {
                const int64_t j = base + tid;
                bool in = false, zero = false;
                uint32_t key = 0u;
                if (j < n_cols) {
                    key = walk2_key(walk2_weight(acc, col_scale, j, diag));
                    in = (key & hi_mask) == prefix;
                    zero = in && key == 0u;
                }
                // the cells nobody reached would all hit one counter: a wave counts its own with a ballot
                const unsigned long long zm = __ballot(zero);
                if (zm && lane == __ffsll((long long)zm) - 1) atomicAdd(&hist[0], __popcll(zm));
                if (in && !zero) atomicAdd(&hist[(key >> shift) & 255], 1);
            }
            __syncthreads();
            // every wave finds the digit for itself: lane l owns the digits 4 l .. 4 l + 3
            const int4 h = *reinterpret_cast<const int4 *>(hist + 4 * lane);
            const int own = h.x + h.y + h.z + h.w;
            int suf = own;
#pragma unroll
            for (int off = 1; off < kWave; off <<= 1) {
                const int t = __shfl_down(suf, off, kWave);
                if (lane + off < kWave) suf += t;
            }
            const int above = suf - own;
            const bool mine = above < krem && krem <= suf;
            int digit = 0, left = krem;
            if (mine) {
                int run = above;
                const int hh[4] = {h.x, h.y, h.z, h.w};
                digit = 4 * lane;
                left = krem - run;
#pragma unroll
                for (int d = 3; d >= 0; --d) {
                    if (run + hh[d] >= krem) { digit = 4 * lane + d; left = krem - run; break; }
                    run += hh[d];
                }
            }
            const unsigned long long mm = __ballot(mine);
            const int src = mm ? __ffsll((long long)mm) - 1 : 0;
            digit = __shfl(digit, src, kWave);
            krem = __shfl(left, src, kWave);
            prefix |= (uint32_t)digit << shift;
        }
        // prefix: the key of the keff-th largest weight; krem of the entries with that key are taken, lowest columns
        // first.  The key 0 (nothing positive left) is never kept.
        const uint32_t thr = prefix;
        const int take_eq = thr == 0u ? 0 : krem;
        int run_gt = 0, run_eq = 0, par = 0;
        for (int64_t base = 0; base < n_cols; base += kBlock) {
            const int64_t j = base + tid;
            float w = 0.f;
            bool gt = false, eq = false;
            if (j < n_cols) {
                w = walk2_weight(acc, col_scale, j, diag);
                acc[j] = 0.f;                                   // the last read of this cell: cleared for the next row
                const uint32_t key = walk2_key(w);
                gt = key > thr;
                eq = key == thr;
            }
            const unsigned long long gm = __ballot(gt), em = __ballot(eq);
            if (lane == 0) { s_cnt[par][wave][0] = __popcll(gm); s_cnt[par][wave][1] = __popcll(em); }
            __syncthreads();
            int gt_before = run_gt + __popcll(gm & below), eq_before = run_eq + __popcll(em & below);
            int gt_all = 0, eq_all = 0;
#pragma unroll
            for (int wv = 0; wv < kW2Waves; ++wv) {
                const int cg = s_cnt[par][wv][0], ce = s_cnt[par][wv][1];
                if (wv < wave) { gt_before += cg; eq_before += ce; }
                gt_all += cg;
                eq_all += ce;
            }
            par ^= 1;
            if (gt || (eq && eq_before < take_eq)) {
                const int slot = gt_before + (eq_before < take_eq ? eq_before : take_eq);
                if (slot < K) { s_col[slot] = (int32_t)j; s_val[slot] = w; }          // (always: slot < keff <= K)
            }
            run_gt += gt_all;
            run_eq += eq_all;
        }
        const int kept = run_gt + (run_eq < take_eq ? run_eq : take_eq);
        __syncthreads();
        if (normalize) {
            if (tid == 0) {
                float s = 0.f;
                for (int sidx = 0; sidx < kept; ++sidx) s = s + s_val[sidx];      // ascending column
                s_sum = s;
            }
            __syncthreads();
        }
        int32_t *out_col = cols + i * K;
        float *out_val = vals + i * K;
        for (int sidx = tid; sidx < K; sidx += kBlock) {
            const bool used = sidx < kept;
            float v = used ? s_val[sidx] : 0.f;
            if (used && normalize) v = __fdiv_rn(v, s_sum);
            out_col[sidx] = used ? s_col[sidx] : -1;
            out_val[sidx] = v;
        }
        if (tid == 0) count[i] = kept;
        __syncthreads();                                        // s_row, s_hist and the kept pairs are free again
    }
}

}  // namespace
}  // namespace daisy

using namespace daisy;

extern "C" {

size_t daisy_walk2_workspace_bytes(int64_t n_rows, int64_t n_cols, int32_t path, int32_t n_groups) {
    if (n_rows < 0 || n_cols < 1 || n_cols > INT_MAX || path < DAISY_SLIM_PATH_AUTO || path > DAISY_SLIM_PATH_GLOBAL ||
        n_groups < 0 || n_groups > kW2MaxGroups)
        return 0;
    const bool lds = walk2_lds(path, n_cols);
    if (lds) return kW2CounterBytes;
    return kW2CounterBytes + (size_t)walk2_groups(n_rows, n_cols, false, n_groups) * walk2_slab_bytes(n_cols);
}

int daisy_walk2_topk(const int64_t *a_ptr, const int32_t *a_col, const float *a_val, int64_t n_rows, int64_t inner,
                     const int64_t *b_ptr, const int32_t *b_col, const float *b_val, int64_t n_cols, const float *col_scale,
                     int32_t zero_diagonal, int32_t normalize, int32_t K, int32_t *count, int32_t *cols, float *vals,
                     int32_t path, int32_t n_groups, void *workspace, size_t workspace_bytes, daisy_stream_t stream) {
    DAISY_CHECK_ARG(K >= 1 && K <= DAISY_KNN_MAX_K, "walk2_topk: K=%d outside [1, %d]", K, DAISY_KNN_MAX_K);
    DAISY_CHECK_ARG(a_ptr && a_col && a_val && b_ptr && b_col && b_val && count && cols && vals && workspace,
                    "walk2_topk: NULL argument");
    DAISY_CHECK_ARG(n_rows >= 0 && n_rows <= INT_MAX && inner >= 1 && inner <= INT_MAX && n_cols >= 1 && n_cols <= INT_MAX,
                    "walk2_topk: n_rows=%lld inner=%lld n_cols=%lld", (long long)n_rows, (long long)inner, (long long)n_cols);
    DAISY_CHECK_ARG(path >= DAISY_SLIM_PATH_AUTO && path <= DAISY_SLIM_PATH_GLOBAL, "walk2_topk: path=%d", path);
    DAISY_CHECK_ARG(n_groups >= 0 && n_groups <= kW2MaxGroups, "walk2_topk: n_groups=%d outside [0, %d]", n_groups,
                    kW2MaxGroups);
    const bool lds = walk2_lds(path, n_cols);
    DAISY_CHECK_ARG(!lds || n_cols <= DAISY_WALK2_LDS_COLS, "walk2_topk: the LDS path holds at most %d columns (n_cols=%lld)",
                    DAISY_WALK2_LDS_COLS, (long long)n_cols);
    const size_t need = daisy_walk2_workspace_bytes(n_rows, n_cols, path, n_groups);
    DAISY_CHECK_ARG(workspace_bytes >= need, "walk2_topk: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if (n_rows == 0) return DAISY_OK;
    const int groups = walk2_groups(n_rows, n_cols, lds, n_groups);
    hipStream_t s = as_stream(stream);
    unsigned long long *next_row = static_cast<unsigned long long *>(workspace);
    float *slabs = reinterpret_cast<float *>(static_cast<char *>(workspace) + kW2CounterBytes);
    const size_t pitch = walk2_slab_bytes(n_cols) / sizeof(float);
    DAISY_HIP(hipMemsetAsync(next_row, 0, kW2CounterBytes, s));
    if (lds) {
        // set on every launch: the attribute belongs to the device's copy of the kernel, not to the process
        DAISY_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_walk2_topk<true>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, DAISY_WALK2_LDS_COLS * (int)sizeof(float)));
        hipLaunchKernelGGL(k_walk2_topk<true>, dim3((unsigned)groups), dim3(kBlock), (size_t)n_cols * sizeof(float), s, a_ptr,
                           a_col, a_val, n_rows, inner, b_ptr, b_col, b_val, n_cols, col_scale, (int)(zero_diagonal != 0),
                           (int)(normalize != 0), (int)K, count, cols, vals, next_row, (float *)nullptr, (size_t)0);
    } else {
        hipLaunchKernelGGL(k_walk2_topk<false>, dim3((unsigned)groups), dim3(kBlock), 0, s, a_ptr, a_col, a_val, n_rows, inner,
                           b_ptr, b_col, b_val, n_cols, col_scale, (int)(zero_diagonal != 0), (int)(normalize != 0), (int)K,
                           count, cols, vals, next_row, slabs, pitch);
    }
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // extern "C"
