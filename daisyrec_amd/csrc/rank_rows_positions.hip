// Exact ranks of held-out items over rows of fp32 scores: full_rank_positions of the models whose
// score comes out of a kernel of its own (NFM, Multi-VAE; NeuMF's at the ops level), and of anyone holding a score matrix.
//   k_rank_rows_positions_f32   one kBlock workgroup per row.  It takes the row's targets in blocks of kRcTc: a target is
//                       range-checked, searched in the row's exclusion list, and its sort word (rank_key_f32.h: section 24's
//                       order-preserving score key | 0xFFFFFFFF - item) is built from the row's own stored value; the
//                       ranked words are sorted largest first in LDS.  Then the row streams by as in k_rank_rows_f32 -
//                       steps of kRrpStep items, four consecutive items per thread (one float4 when the rows allow it),
//                       the next step's loads issued before this step's barrier, the exclusion walked forward into an
//                       LDS mask - and every item that is not excluded is counted into the bucket of rank_count.h.  A row
//                       of more than kRcTc targets reads the score row once per block.
// Order: score descending, a NaN first, -0.0 equal to +0.0, equal scores by ascending item id - k_rank_rows_f32's, so that
// with the same arguments its ids[r][pos] is the target.  No workspace, no global atomics, no floating-point atomics: two
// runs give the same bits.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "rank_count.h"
#include "rank_key_f32.h"

namespace daisy {
namespace {

constexpr int kRrpPer = 4;                         // consecutive items of a thread per step: one float4
constexpr int kRrpStep = kBlock * kRrpPer;         // items per step

struct RrpOrd {                                    // a larger word ranks before a smaller one; no candidate maps to word 0
    static __device__ __forceinline__ bool before(const uint64_t &a, const uint64_t &b) { return a > b; }
    static __device__ __forceinline__ uint64_t pad() { return 0ull; }
};
struct RrpState {
    RcState<uint64_t> rc;
    uint32_t mask[2][kRrpStep / 32];               // step s uses mask s & 1: a step needs no closing barrier
};

// VEC: scores is 16-byte aligned and pitch % 4 == 0, so a thread's four items of a whole step are one float4
template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_rank_rows_positions_f32(
    const float *__restrict__ scores, int64_t I, int64_t pitch, const int64_t *__restrict__ row_users,
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ eitems, const int64_t *__restrict__ t_indptr,
    const int32_t *__restrict__ t_items, const int64_t *__restrict__ out_indptr, int64_t n_targets,
    int32_t *__restrict__ out_pos, float *__restrict__ out_scores, int32_t *__restrict__ out_eligible) {
    __shared__ RrpState st;
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const float *__restrict__ row = scores + r * pitch;
    const int64_t u = row_users[r];
    const int64_t ex_lo = eitems ? indptr[u] : 0, ex_hi = eitems ? indptr[u + 1] : 0;
    const int64_t t_lo = t_indptr[u], dst0 = out_indptr[r];
    int64_t t_len = out_indptr[r + 1] - dst0;               // the caller's row length, never more than the target row's
    if (t_len > t_indptr[u + 1] - t_lo) t_len = t_indptr[u + 1] - t_lo;
    if (t_len <= 0 && !out_eligible) return;                // (uniform) nothing to write
    // No load reads past the row's item_num values: a whole step is one float4 per thread, the step at the row's end
    // (and every step of the scalar form) element by element with the index clamped to the last item.
    auto load = [&](int64_t c0, float (&o)[kRrpPer]) {
        const int64_t i0 = c0 + (int64_t)tid * kRrpPer;
        if (VEC && c0 + kRrpStep <= I) {                    // (uniform)
            const float4 q = *reinterpret_cast<const float4 *>(row + i0);
            o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
        } else {
#pragma unroll
            for (int x = 0; x < kRrpPer; ++x) o[x] = row[i0 + x < I ? i0 + x : I - 1];
        }
    };
    for (int64_t blk = 0; blk == 0 || blk < t_len; blk += kRcTc) {
        const int len = (int)(t_len - blk < kRcTc ? (t_len - blk > 0 ? t_len - blk : 0) : kRcTc);
        for (int e = tid; e <= kRcTc; e += kBlock) st.rc.bucket[e] = 0;
        if (tid == 0) st.rc.cnt = 0;
        __syncthreads();
        // the block's targets: two per thread.  A word of 0: not ranked (or no target)
        uint64_t mine[2];
        float mine_s[2];
        bool has[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int e = tid + q * kBlock;
            has[q] = e < len;
            mine[q] = 0ull;
            mine_s[q] = -INFINITY;
            if (has[q]) {
                const int64_t t = (int64_t)t_items[t_lo + blk + e];
                bool ok = t >= 0 && t < I;                  // checked before it indexes anything
                if (ok && eitems) {
                    int64_t a = ex_lo, z = ex_hi;
                    while (a < z) {
                        const int64_t m = a + (z - a) / 2;
                        if ((int64_t)eitems[m] < t) a = m + 1; else z = m;
                    }
                    ok = !(a < ex_hi && (int64_t)eitems[a] == t);
                }
                if (ok) {
                    mine_s[q] = row[t];                     // the row's own stored value, with its bits
                    mine[q] = fr_word(mine_s[q], t);
                    st.rc.tgt[atomicAdd(&st.rc.cnt, 1)] = mine[q];          // (at most len <= kRcTc entries)
                }
            }
        }
        __syncthreads();
        const int c = st.rc.cnt;
        if (c > 1) rc_sort<RrpOrd>(st.rc.tgt, c);           // (uniform)
        int64_t cur = ex_lo;
        int par = 0;
        float v[kRrpPer], nx[kRrpPer] = {0.f, 0.f, 0.f, 0.f};
        load(0, v);
        for (int64_t c0 = 0; c0 < I; c0 += kRrpStep, par ^= 1) {
            const int64_t c1 = c0 + kRrpStep;
            if (c1 < I) load(c1, nx);                       // (uniform) in flight across this step's barriers
            uint32_t ex = 0u;                               // bit x: item c0 + 4 tid + x is excluded
            if (eitems) {                                   // (uniform)
                uint32_t *mask = st.mask[par];
                if (tid < kRrpStep / 32) mask[tid] = 0u;
                __syncthreads();
                for (;;) {                                  // at most (ex_hi - cur) / kBlock + 1 rounds
                    const int64_t p = cur + tid;
                    const bool in_row = p < ex_hi;
                    const int64_t e = in_row ? (int64_t)eitems[p] : c1;
                    if (e >= c0 && e < c1) atomicOr(&mask[(int)(e - c0) >> 5], 1u << ((int)(e - c0) & 31));
                    const int below = __syncthreads_count(in_row && e < c1);      // an ascending row: a prefix of the window
                    cur += below;                                                 // (never past ex_hi: only in_row entries count)
                    if (below < kBlock) break;
                }
                ex = (mask[tid >> 3] >> ((tid & 7) * kRrpPer)) & 0xFu;
            }
            const int64_t i0 = c0 + (int64_t)tid * kRrpPer;
            bool on[kRrpPer];
            int g[kRrpPer];
#pragma unroll
            for (int x = 0; x < kRrpPer; ++x) {             // four independent searches
                on[x] = i0 + x < I && !((ex >> x) & 1u);
                g[x] = on[x] ? rc_before_count<RrpOrd>(st.rc.tgt, c, fr_word(v[x], i0 + x)) : 0;
            }
            if (c < kRcFew) {                               // (uniform)
                rc_bucket_add_few<kRrpPer>(st.rc.bucket, on, g, c);
            } else {
#pragma unroll
                for (int x = 0; x < kRrpPer; ++x) rc_bucket_add(st.rc.bucket, on[x], g[x]);
            }
#pragma unroll
            for (int x = 0; x < kRrpPer; ++x) v[x] = nx[x];
        }
        const int eligible = rc_positions(st.rc, c);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int64_t dst = dst0 + blk + tid + q * kBlock;
            if (has[q] && dst >= 0 && dst < n_targets) {
                out_pos[dst] = mine[q] ? st.rc.bucket[rc_before_count<RrpOrd>(st.rc.tgt, c, mine[q])] : -1;
                if (out_scores) out_scores[dst] = mine_s[q];
            }
        }
        if (blk == 0 && out_eligible && tid == 0) out_eligible[r] = eligible;
        __syncthreads();                                    // the next block rewrites the state
    }
}

}  // namespace
}  // namespace daisy

using namespace daisy;

extern "C" {

int daisy_rank_rows_positions_f32(const float *scores, int64_t m, int64_t item_num, int64_t pitch, const int64_t *row_users,
                                  const int64_t *excl_indptr, const int32_t *excl_items, const int64_t *tgt_indptr,
                                  const int32_t *tgt_items, const int64_t *out_indptr, int64_t n_targets, int32_t *out_pos,
                                  float *out_scores, int32_t *out_eligible, daisy_stream_t stream) {
    const char *what = "rank_rows_positions_f32";
    DAISY_CHECK_ARG(m >= 0 && m <= INT_MAX, "%s: bad row count m=%lld", what, (long long)m);
    DAISY_CHECK_ARG(n_targets >= 0, "%s: bad target count n_targets=%lld", what, (long long)n_targets);
    DAISY_CHECK_ARG(m == 0 || (scores && row_users && tgt_indptr && out_indptr),
                    "%s: NULL argument (scores, row_users, tgt_indptr, out_indptr)", what);
    DAISY_CHECK_ARG(m == 0 || n_targets == 0 || (tgt_items && out_pos), "%s: NULL argument (tgt_items, out_pos)", what);
    DAISY_CHECK_ARG(item_num >= 1 && item_num <= INT_MAX, "%s: item_num=%lld outside [1, 2^31)", what, (long long)item_num);
    DAISY_CHECK_ARG(pitch >= item_num, "%s: pitch=%lld below item_num=%lld", what, (long long)pitch, (long long)item_num);
    DAISY_CHECK_ARG((excl_indptr != nullptr) == (excl_items != nullptr),
                    "%s: excl_indptr and excl_items are given together or not at all", what);
    if (m == 0 || (n_targets == 0 && !out_eligible)) return DAISY_OK;
    const bool vec = reinterpret_cast<uintptr_t>(scores) % 16 == 0 && pitch % 4 == 0;      // chosen once per launch
    auto kern = vec ? k_rank_rows_positions_f32<true> : k_rank_rows_positions_f32<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)m), dim3(kBlock), 0, as_stream(stream), scores, item_num, pitch, row_users,
                       excl_indptr, excl_items, tgt_indptr, tgt_items, out_indptr, n_targets, out_pos, out_scores, out_eligible);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // extern "C"
