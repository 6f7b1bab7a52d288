// Masked streaming top-k over rows of fp32 scores: the selector behind full_rank_users of the
// models whose score comes out of a kernel of its own (NeuMF, NFM, Multi-VAE), and of anyone holding a score matrix.
//   k_rank_rows_f32     one kBlock workgroup per row walks the row in steps of kRrStep items, four consecutive items per
//                       thread (one float4 when the rows allow it).  A value is dropped when its item is in the row's
//                       exclusion list or when a float compare shows that it cannot beat the k-th best candidate so
//                       far; what is left becomes section 24's 64-bit sort word (order-preserving score key | 0xFFFFFFFF -
//                       item), is tested exactly and appended to a candidate buffer in LDS - one LDS atomic per wave
//                       claims the places.  A buffer that could not take another whole step is sorted by a bitonic
//                       network in LDS, cut to its topk largest words, and the threshold rises.  The next step's
//                       loads are issued before the current step's barrier.
// The order on sort words is total (score descending, a NaN first, -0.0 equal to +0.0, item ascending), so the top-k SET
// of a row is unique: the result depends neither on the append order nor on wave scheduling, and two runs give the same
// bits.  No workspace, no global atomics, no floating-point atomics.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "rank_key_f32.h"

namespace daisy {
namespace {

constexpr int kRrTopkCap = 128;                    // the contract's cap (as section 24's)
constexpr int kRrPer = 4;                          // consecutive items of a thread per step: one float4
constexpr int kRrStep = kBlock * kRrPer;           // items per step
constexpr int kRrBuf = kRrTopkCap + kRrStep;       // candidate words: a compacted buffer plus one whole step
constexpr int kRrLimit = kRrBuf - kRrStep;         // a buffer holding more than this is compacted before the next step
static_assert(kRrLimit >= kRrTopkCap, "a compacted buffer must leave room for one step");

struct RrState {
    uint64_t word[kRrBuf];
    uint32_t mask[kRrStep / 32];                   // bit = item of the step is in the row's exclusion list
    int cnt;
};
constexpr int kRrLdsBytes = (int)sizeof(RrState);  // 9352 (9616 with the barrier reductions' words)
static_assert(8 * (kRrLdsBytes + 512) <= 160 * 1024, "the wave slots (8 workgroups per CU), not the LDS, bound the occupancy");

// one comparator of the network: the larger word to the lower place.  Places at or past kRrBuf do not exist: they stand
// for empty words (0, the minimum), which a comparator that only ever moves the larger word DOWN leaves where they are.
__device__ __forceinline__ void rr_cmpx(RrState &st, int i, int l) {
    if (l >= kRrBuf) return;
    const uint64_t a = st.word[i], b = st.word[l];
    if (b > a) { st.word[i] = b; st.word[l] = a; }
}

// Called by every thread with the same c <= kRrBuf: the first c words, largest first.  A bitonic network over the next
// power of two n2 >= c in its one-direction form (a mirrored first stage per merge, then half-cleaners), so that the
// padding - real zero words up to min(n2, kRrBuf), virtual ones beyond - stays at the end through every stage.
__device__ __forceinline__ void rr_sort(RrState &st, int c) {
    const int tid = threadIdx.x;
    int n2 = 2;
    while (n2 < c) n2 <<= 1;
    const int top = n2 < kRrBuf ? n2 : kRrBuf;
    for (int e = c + tid; e < top; e += kBlock) st.word[e] = 0ull;
    __syncthreads();
    const int half = n2 >> 1;
    for (int k = 2; k <= n2; k <<= 1) {
        for (int t = tid; t < half; t += kBlock) {          // place o of a block of k against place k - 1 - o
            const int o = t & ((k >> 1) - 1);
            const int i = ((t - o) << 1) | o;
            rr_cmpx(st, i, i + k - 1 - 2 * o);
        }
        __syncthreads();
        for (int j = k >> 2; j >= 1; j >>= 1) {
            for (int t = tid; t < half; t += kBlock) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                rr_cmpx(st, i, i | j);
            }
            __syncthreads();
        }
    }
}

// VEC: scores is 16-byte aligned and pitch % 4 == 0, so a thread's four items of a whole step are one float4
template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_rank_rows_f32(const float *__restrict__ scores, int64_t I, int64_t pitch,
                                                          const int64_t *__restrict__ row_users,
                                                          const int64_t *__restrict__ indptr,
                                                          const int32_t *__restrict__ eitems, int topk,
                                                          int64_t *__restrict__ out_ids, float *__restrict__ out_scores) {
    __shared__ RrState st;
    const int tid = threadIdx.x, lane = tid % kWave;
    const int64_t r = blockIdx.x;
    const float *__restrict__ row = scores + r * pitch;
    int64_t cur = 0, ex_hi = 0;                             // the row's exclusion list: a cursor that only moves forward
    if (eitems) {
        const int64_t u = row_users[r];
        cur = indptr[u];
        ex_hi = indptr[u + 1];
    }
    if (tid == 0) st.cnt = 0;
    // No load reads past the row's item_num values: a whole step is one float4 per thread, the step at the row's end
    // (and every step of the scalar form) element by element with the index clamped to the last item.
    auto load = [&](int64_t c0, float (&o)[kRrPer]) {
        const int64_t i0 = c0 + (int64_t)tid * kRrPer;
        if (VEC && c0 + kRrStep <= I) {                     // (uniform)
            const float4 q = *reinterpret_cast<const float4 *>(row + i0);
            o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
        } else {
#pragma unroll
            for (int x = 0; x < kRrPer; ++x) o[x] = row[i0 + x < I ? i0 + x : I - 1];
        }
    };
    uint64_t thr = 0ull;                                    // the topk-th best word so far; 0: none yet
    float thr_f = -INFINITY;                                // its score: what does not reach it needs no word
    float v[kRrPer], nx[kRrPer] = {0.f, 0.f, 0.f, 0.f};
    load(0, v);
    __syncthreads();
    for (int64_t c0 = 0; c0 < I; c0 += kRrStep) {
        const int64_t c1 = c0 + kRrStep;
        if (c1 < I) load(c1, nx);                           // (uniform) in flight across this step's barriers
        uint32_t ex = 0u;                                   // bit x: item c0 + 4 tid + x is excluded
        if (eitems) {                                       // (uniform)
            if (tid < kRrStep / 32) st.mask[tid] = 0u;
            __syncthreads();
            for (;;) {                                      // at most (ex_hi - cur) / kBlock + 1 rounds
                const int64_t p = cur + tid;
                const bool in_row = p < ex_hi;
                const int64_t e = in_row ? (int64_t)eitems[p] : c1;
                if (e >= c0 && e < c1) atomicOr(&st.mask[(int)(e - c0) >> 5], 1u << ((int)(e - c0) & 31));
                const int below = __syncthreads_count(in_row && e < c1);      // an ascending row: a prefix of the window
                cur += below;                                                 // (never past ex_hi: only in_row entries count)
                if (below < kBlock) break;
            }
            ex = (st.mask[tid >> 3] >> ((tid & 7) * kRrPer)) & 0xFu;
        }
        const int64_t i0 = c0 + (int64_t)tid * kRrPer;
        uint32_t pre = 0u;
#pragma unroll
        for (int x = 0; x < kRrPer; ++x)
            pre |= (i0 + x < I && !((ex >> x) & 1u) && !(v[x] < thr_f)) ? (1u << x) : 0u;       // (a NaN passes)
        int full = 0;
        if (__ballot(pre != 0u)) {                          // (uniform over the wave)
            uint64_t w[kRrPer];
            unsigned long long bal[kRrPer];
            int tot = 0;
#pragma unroll
            for (int x = 0; x < kRrPer; ++x) {
                w[x] = fr_word(v[x], i0 + x);
                bal[x] = __ballot(((pre >> x) & 1u) && w[x] > thr);
                tot += __popcll(bal[x]);
            }
            if (tot) {                                      // (uniform over the wave) one claim of places per wave
                int base = 0;
                if (lane == 0) base = atomicAdd(&st.cnt, tot);
                base = __shfl(base, 0, kWave);
                full = base + tot > kRrLimit;               // the wave that adds last sees the step's final count
                const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
                for (int x = 0; x < kRrPer; ++x) {
                    const int pos = base + __popcll(bal[x] & lt);
                    if (((bal[x] >> lane) & 1ull) && pos < kRrBuf) st.word[pos] = w[x];      // (always: <= kRrLimit before the step)
                    base += __popcll(bal[x]);
                }
            }
        }
        if (__syncthreads_or(full)) {                       // the buffer could not take another whole step
            const int n = st.cnt;                           // (the next claim is behind the barriers below)
            const int c = n < kRrBuf ? n : kRrBuf;
            rr_sort(st, c);
            thr = (c >= topk) ? st.word[topk - 1] : 0ull;
            thr_f = thr ? fr_word_score(thr) : -INFINITY;
            if (tid == 0) st.cnt = c < topk ? c : topk;
            __syncthreads();
        }
#pragma unroll
        for (int x = 0; x < kRrPer; ++x) v[x] = nx[x];
    }
    const int n = st.cnt;
    const int c = n < kRrBuf ? n : kRrBuf;
    if (c > 1) rr_sort(st, c);                              // (uniform)
    if (tid < topk) {
        const bool has = tid < c;
        const int64_t id = has ? fr_word_item(st.word[has ? tid : 0]) : (int64_t)-1;
        out_ids[r * topk + tid] = id;
        // the row's own stored value, not the key decoded: the bits of the score kernel (a NaN's payload, the sign of a zero)
        if (out_scores) out_scores[r * topk + tid] = has ? row[id] : -INFINITY;
    }
}

}  // namespace
}  // namespace daisy

using namespace daisy;

extern "C" {

int daisy_rank_rows_f32(const float *scores, int64_t m, int64_t item_num, int64_t pitch, const int64_t *row_users,
                        const int64_t *excl_indptr, const int32_t *excl_items, int32_t topk, int64_t *out_ids,
                        float *out_scores, daisy_stream_t stream) {
    DAISY_CHECK_ARG(m >= 0 && m <= INT_MAX, "rank_rows_f32: bad row count m=%lld", (long long)m);
    DAISY_CHECK_ARG(m == 0 || (scores && out_ids), "rank_rows_f32: NULL argument (scores, out_ids)");
    DAISY_CHECK_ARG(item_num >= 1 && item_num <= INT_MAX, "rank_rows_f32: item_num=%lld outside [1, 2^31)", (long long)item_num);
    DAISY_CHECK_ARG(pitch >= item_num, "rank_rows_f32: pitch=%lld below item_num=%lld", (long long)pitch, (long long)item_num);
    DAISY_CHECK_ARG((excl_indptr != nullptr) == (excl_items != nullptr),
                    "rank_rows_f32: excl_indptr and excl_items are given together or not at all");
    DAISY_CHECK_ARG(!excl_indptr || row_users, "rank_rows_f32: an exclusion needs row_users (the CSR row of every score row)");
    DAISY_CHECK_ARG(topk <= kRrTopkCap, "rank_rows_f32: topk=%d above the cap of %d (the candidate buffer lives in LDS)", topk,
                    kRrTopkCap);
    DAISY_CHECK_ARG(topk >= 1 && topk <= item_num, "rank_rows_f32: topk=%d outside [1, item_num=%lld]", topk,
                    (long long)item_num);
    if (m == 0) return DAISY_OK;
    const bool vec = reinterpret_cast<uintptr_t>(scores) % 16 == 0 && pitch % 4 == 0;      // chosen once per launch
    auto kern = vec ? k_rank_rows_f32<true> : k_rank_rows_f32<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)m), dim3(kBlock), 0, as_stream(stream), scores, item_num, pitch, row_users,
                       excl_indptr, excl_items, (int)topk, out_ids, out_scores);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // extern "C"
