// The exact ranks of one request's targets over ALL items on fp64 scores, shared by the entries
// of rank_positions_f64.hip.  One kBlock workgroup per request: it takes the target row in blocks of kRcTc, range-checks,
// exclusion-searches and scores every target of the block, sorts the ranked ones best first in LDS, and then walks the
// items exactly as rank_f64_users_body does - chunks of kBlock, the forward walk of the exclusion row into an LDS mask,
// one score per thread - counting every eligible item into the bucket of rank_count.h.  A row longer than kRcTc scores
// the items once per block.  No score row and no list is ever written.
//
// Order (rank_f64_users.h's): the key of v + 0.0 descending, equal keys by ascending item id, a NaN is never ranked - not
// as a target (position -1, the NaN returned as its score) and not as an item (neither counted nor eligible).
#pragma once

#include <math.h>

#include "common.h"
#include "rank_count.h"
#include "rank_f64_users.h"

namespace daisy {

struct RpEnt {
    uint64_t key;                                  // rf_key of the score
    uint32_t id;
};
struct RpOrd {
    static __device__ __forceinline__ bool before(const RpEnt &a, const RpEnt &b) { return rf_before(a.key, a.id, b.key, b.id); }
    static __device__ __forceinline__ RpEnt pad() { return RpEnt{0ull, 0xFFFFFFFFu}; }      // (no score maps to key 0)
};
struct RpState {
    RcState<RpEnt> rc;
    uint32_t mask[2][kRfChunk / 32];               // chunk c uses mask c & 1: a chunk without candidates needs no closing barrier
};
constexpr int kRpLdsBytes = (int)sizeof(RpState);

// Scorer: as rank_f64_users_body's.  [ex_lo, ex_hi): the user's row of eitems (NULL: none), only ever compared.
// t_items[t_lo .. t_lo + t_len): the request's targets; their results go to out_pos / out_scores [dst0 .. dst0 + t_len),
// never at or past n_targets.  out_eligible: this request's place, or NULL.
template <class Scorer, class OutT>
__device__ __forceinline__ void rank_f64_positions_body(const Scorer &sc, int64_t I, const int32_t *__restrict__ eitems,
                                                        int64_t ex_lo, int64_t ex_hi, const int32_t *__restrict__ t_items,
                                                        int64_t t_lo, int64_t t_len, int64_t dst0, int64_t n_targets,
                                                        int32_t *__restrict__ out_pos, OutT *__restrict__ out_scores,
                                                        int32_t *__restrict__ out_eligible) {
    __shared__ RpState st;
    const int tid = threadIdx.x;
    if (t_len <= 0 && !out_eligible) return;                // (uniform) nothing to write
    for (int64_t blk = 0; blk == 0 || blk < t_len; blk += kRcTc) {
        const int len = (int)(t_len - blk < kRcTc ? (t_len - blk > 0 ? t_len - blk : 0) : kRcTc);
        for (int e = tid; e <= kRcTc; e += kBlock) st.rc.bucket[e] = 0;
        if (tid == 0) st.rc.cnt = 0;
        __syncthreads();
        // the block's targets: two per thread.  state -1: no target, 0: not ranked, 1: ranked
        RpEnt mine[2];
        double mine_s[2];
        int state[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int e = tid + q * kBlock;
            state[q] = -1;
            mine[q] = RpOrd::pad();
            mine_s[q] = -INFINITY;
            if (e < len) {
                state[q] = 0;
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
                    const double s = sc.score(t);           // the call of the stream below: its bits
                    mine_s[q] = s;
                    if (s == s) {
                        state[q] = 1;
                        mine[q] = RpEnt{rf_key(s), (uint32_t)t};
                        st.rc.tgt[atomicAdd(&st.rc.cnt, 1)] = mine[q];      // (at most len <= kRcTc entries)
                    }
                }
            }
        }
        __syncthreads();
        const int c = st.rc.cnt;
        if (c > 1) rc_sort<RpOrd>(st.rc.tgt, c);            // (uniform)
        int64_t cur = ex_lo;
        int par = 0;
        for (int64_t c0 = 0; c0 < I; c0 += kRfChunk, par ^= 1) {
            const int64_t c1 = c0 + kRfChunk;
            bool excluded = false;
            if (eitems) {                                   // (uniform)
                uint32_t *mask = st.mask[par];
                if (tid < kRfChunk / 32) mask[tid] = 0u;
                __syncthreads();
                for (;;) {                                  // at most (ex_hi - ex_lo) / kBlock + 1 rounds
                    const int64_t p = cur + tid;
                    const bool in_row = p < ex_hi;
                    const int64_t v = in_row ? (int64_t)eitems[p] : c1;
                    if (v >= c0 && v < c1) atomicOr(&mask[(int)(v - c0) >> 5], 1u << ((int)(v - c0) & 31));
                    const int below = __syncthreads_count(in_row && v < c1);      // an ascending row: a prefix of the window
                    cur += below;                                                 // (never past ex_hi: only in_row entries count)
                    if (below < kBlock) break;
                }
                excluded = (mask[tid >> 5] >> (tid & 31)) & 1u;
            }
            const int64_t it = c0 + tid;
            bool on[1] = {it < I && !excluded};
            int g[1] = {0};
            if (on[0]) {
                const double s = sc.score(it);
                on[0] = s == s;
                if (on[0]) g[0] = rc_before_count<RpOrd>(st.rc.tgt, c, RpEnt{rf_key(s), (uint32_t)it});
            }
            if (c < kRcFew) rc_bucket_add_few<1>(st.rc.bucket, on, g, c);       // (uniform)
            else rc_bucket_add(st.rc.bucket, on[0], g[0]);
        }
        const int eligible = rc_positions(st.rc, c);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int64_t dst = dst0 + blk + tid + q * kBlock;
            if (state[q] >= 0 && dst >= 0 && dst < n_targets) {
                out_pos[dst] = state[q] == 1 ? st.rc.bucket[rc_before_count<RpOrd>(st.rc.tgt, c, mine[q])] : -1;
                if (out_scores) out_scores[dst] = (OutT)mine_s[q];
            }
        }
        if (blk == 0 && out_eligible && tid == 0) *out_eligible = eligible;
        __syncthreads();                                    // the next block rewrites the state
    }
}

}  // namespace daisy
