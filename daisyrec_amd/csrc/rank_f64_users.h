// The streaming top-k of one user over ALL items on fp64 scores, shared by the full rankings of
// rank_full_f64.hip.  One kBlock workgroup per user walks the items in chunks of kBlock: a thread computes its item's
// score into a register, drops it when the item is in the user's exclusion row, when it is not a number or when it does
// not beat the k-th best candidate so far, and otherwise appends (key, id) to a candidate buffer in LDS - one LDS atomic
// per wave claims the places.  A buffer that could not take another whole chunk is sorted in LDS (bitonic network over
// (key, id)), cut to its topk best, and the threshold rises.  No score row is ever written.
//
// Order (topk_f64.h's): score descending compared as fp64, -0.0 equal to +0.0, equal scores by ascending item id, a
// NaN never selected.  A candidate is the order-preserving 64-bit key of v + 0.0 plus the item id: the order is total
// and two candidates of a user never compare equal, so the top-k SET is unique and the result depends neither on the
// append order nor on wave scheduling.
#pragma once

#include <math.h>

#include "common.h"

namespace daisy {

constexpr int kRfTopkCap = 128;                    // the contract's cap (as section 24's)
constexpr int kRfChunk = kBlock;                   // items per step: one per thread
constexpr int kRfBuf = 512;                        // candidate entries; a power of two: the network sorts all of it
constexpr int kRfLimit = kRfBuf - kRfChunk;        // a buffer holding more than this is compacted before the next chunk
static_assert((kRfBuf & (kRfBuf - 1)) == 0 && kRfBuf == 2 * kBlock, "one compare-exchange per thread and step");
static_assert(kRfLimit >= kRfTopkCap, "a compacted buffer must leave room for one chunk");

struct RfState {
    uint64_t key[kRfBuf];
    uint32_t id[kRfBuf];
    uint32_t mask[kRfChunk / 32];                  // bit = item of the chunk is in the exclusion row
    uint64_t thr_key;                              // the k-th best candidate so far; key 0: none yet (no score maps to 0)
    uint32_t thr_id;
    int cnt;
};
constexpr int kRfLdsBytes = (int)sizeof(RfState);

// larger score <-> larger key, for every v that is a number; -0.0 and +0.0 share a key.  -inf maps to 2^52 - 1, so key 0
// is free to mean "nothing".
__device__ __forceinline__ uint64_t rf_key(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v + 0.0);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double rf_unkey(uint64_t key) {
    return __longlong_as_double((long long)((key >> 63) ? (key ^ 0x8000000000000000ull) : ~key));
}
// candidate a ranks before candidate b
__device__ __forceinline__ bool rf_before(uint64_t ak, uint32_t ai, uint64_t bk, uint32_t bi) {
    return ak > bk || (ak == bk && ai < bi);
}

// Called by every thread: the first c entries of the buffer, best first (the places behind them hold key 0).
__device__ __forceinline__ void rf_sort(RfState &st, int c) {
    const int tid = threadIdx.x;
    for (int e = tid; e < kRfBuf; e += kBlock)
        if (e >= c) { st.key[e] = 0ull; st.id[e] = 0xFFFFFFFFu; }
    __syncthreads();
    for (int k = 2; k <= kRfBuf; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            const int i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), l = i | j;          // i < l < kRfBuf
            const uint64_t ka = st.key[i], kb = st.key[l];
            const uint32_t ia = st.id[i], ib = st.id[l];
            const bool best_first = (i & k) == 0;
            if (rf_before(kb, ib, ka, ia) == best_first && !(ka == kb && ia == ib)) {
                st.key[i] = kb; st.id[i] = ib;
                st.key[l] = ka; st.id[l] = ia;
            }
            __syncthreads();
        }
    }
}

// Scorer: `double score(int64_t item) const`, a pure function of the item for this workgroup's user; a value that is not
// a number is never selected.  [ex_lo, ex_hi) is the user's row of the exclusion items (eitems == NULL: none): its
// contents are only compared, the cursor into it only moves forward and never leaves the row.
// out_ids[0 .. topk), out_scores[0 .. topk) or NULL: the user's row of the result.
template <class Scorer, class OutT>
__device__ __forceinline__ void rank_f64_users_body(const Scorer &sc, int64_t I, const int32_t *__restrict__ eitems,
                                                    int64_t ex_lo, int64_t ex_hi, int topk, int64_t *__restrict__ out_ids,
                                                    OutT *__restrict__ out_scores) {
    __shared__ RfState st;
    const int tid = threadIdx.x, lane = tid % kWave;
    if (tid == 0) { st.cnt = 0; st.thr_key = 0ull; st.thr_id = 0xFFFFFFFFu; }
    uint64_t thr_key = 0ull;
    uint32_t thr_id = 0xFFFFFFFFu;
    int64_t cur = ex_lo;
    for (int64_t c0 = 0; c0 < I; c0 += kRfChunk) {
        const int64_t c1 = c0 + kRfChunk;
        if (eitems && tid < kRfChunk / 32) st.mask[tid] = 0u;
        __syncthreads();                                    // also: every thread has read the last chunk's count
        bool excluded = false;
        if (eitems) {                                       // (uniform)
            for (;;) {                                      // at most (ex_hi - ex_lo) / kBlock + 1 rounds
                const int64_t p = cur + tid;
                const bool in_row = p < ex_hi;
                const int64_t v = in_row ? (int64_t)eitems[p] : c1;
                if (v >= c0 && v < c1) atomicOr(&st.mask[(int)(v - c0) >> 5], 1u << ((int)(v - c0) & 31));
                const int below = __syncthreads_count(in_row && v < c1);      // an ascending row: a prefix of the window
                cur += below;                                                 // (never past ex_hi: only in_row entries count)
                if (below < kBlock) break;
            }
            excluded = (st.mask[tid >> 5] >> (tid & 31)) & 1u;
        }
        const int64_t it = c0 + tid;
        bool pass = false;
        uint64_t key = 0ull;
        if (it < I && !excluded) {
            const double s = sc.score(it);
            if (s == s) {
                key = rf_key(s);
                pass = rf_before(key, (uint32_t)it, thr_key, thr_id);
            }
        }
        const unsigned long long bal = __ballot(pass);
        if (bal) {                                          // (uniform over the wave) one claim of places per wave
            int base = 0;
            if (lane == 0) base = atomicAdd(&st.cnt, __popcll(bal));
            base = __shfl(base, 0, kWave);
            const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
            if (pass && pos < kRfBuf) {                     // (always: the count was <= kRfLimit before the chunk)
                st.key[pos] = key;
                st.id[pos] = (uint32_t)it;
            }
        }
        __syncthreads();
        const int c = st.cnt;                               // (uniform: the next claim is behind the barrier above)
        if (c > kRfLimit) {
            rf_sort(st, c < kRfBuf ? c : kRfBuf);
            if (tid == 0) {
                st.cnt = c < topk ? c : topk;
                if (c >= topk) { st.thr_key = st.key[topk - 1]; st.thr_id = st.id[topk - 1]; }
            }
            __syncthreads();
            thr_key = st.thr_key;
            thr_id = st.thr_id;
        }
    }
    __syncthreads();
    const int c = st.cnt < kRfBuf ? st.cnt : kRfBuf;
    __syncthreads();
    rf_sort(st, c);
    for (int t = tid; t < topk; t += kBlock) {
        const bool has = t < c;
        out_ids[t] = has ? (int64_t)st.id[t] : (int64_t)-1;
        if (out_scores) out_scores[t] = has ? (OutT)rf_unkey(st.key[t]) : (OutT)(-INFINITY);
    }
}

}  // namespace daisy
