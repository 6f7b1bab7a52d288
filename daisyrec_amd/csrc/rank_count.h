// Counting the exact ranks of a block of targets while the items of a user stream by, shared by
// rank_f64_positions.h (fp64 scores) and rank_rows_positions.hip (rows of fp32 scores).  One kBlock workgroup holds up to
// kRcTc ranked targets sorted best first in LDS.  An eligible item x looks up g(x), the number of block targets strictly
// before x, by binary search and adds one to bucket g(x); afterwards target r (sorted order) has
//   pos[r] = (bucket[0] + ... + bucket[r]) - 1
// because x comes before target r exactly when x is not that target and g(x) <= r, and the target itself - an eligible
// item like any other - lands in bucket r.  The buckets' total is the number of eligible items.  The work per item is one
// search of at most log2(kRcTc) + 1 steps whatever the row length; the counts are integers, so the result depends neither
// on the order of the additions nor on wave scheduling.
//
// Ord: `static bool before(const Ent &a, const Ent &b)`, a strict total order on the entries that can occur, and
// `static Ent pad()`, an entry no real one comes after.
#pragma once

#include "common.h"

namespace daisy {

constexpr int kRcTc = 512;                         // targets of a block; a power of two: the network sorts up to all of it
constexpr int kRcAgg = 8;                          // buckets a wave adds to with one atomic each before its lanes add alone
constexpr int kRcFew = 16;                         // below this many ranked targets a wave counts bucket by bucket
static_assert(kRcFew <= kWave, "lane k carries the count of bucket k");
static_assert((kRcTc & (kRcTc - 1)) == 0 && kRcTc == 2 * kBlock, "the scan takes two buckets per thread");

template <class Ent>
struct RcState {
    Ent tgt[kRcTc];                                // the block's ranked targets, best first
    int bucket[kRcTc + 1];                         // bucket[g]: eligible items with g block targets strictly before them
    int scan[kBlock];
    int cnt;                                       // ranked targets of the block
};

// Called by every thread with the same c <= kRcTc: the first c entries, best first.  A bitonic network over the next
// power of two; the padding ends up behind the entries.
template <class Ord, class Ent>
__device__ __forceinline__ void rc_sort(Ent *a, int c) {
    const int tid = threadIdx.x;
    int n2 = 2;
    while (n2 < c) n2 <<= 1;
    for (int e = c + tid; e < n2; e += kBlock) a[e] = Ord::pad();
    __syncthreads();
    const int half = n2 >> 1;
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int t = tid; t < half; t += kBlock) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;           // i < l < n2
                const Ent x = a[i], y = a[l];
                const bool best_first = (i & k) == 0;
                if (best_first ? Ord::before(y, x) : Ord::before(x, y)) { a[i] = y; a[l] = x; }
            }
            __syncthreads();
        }
    }
}

// entries of a[0 .. c) strictly before x
template <class Ord, class Ent>
__device__ __forceinline__ int rc_before_count(const Ent *a, int c, const Ent &x) {
    int lo = 0, hi = c;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (Ord::before(a[mid], x)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Called by every lane of the wave: bucket[g] += 1 for every lane with `on`.  Lanes that share a bucket share one atomic:
// the first open lane's bucket is added to once with the number of lanes holding it, up to kRcAgg times (a row with few
// targets has few buckets, and most items of any row fall behind the last target); lanes still open then add alone.
// Blocks of fewer than kRcFew targets - the ten held-out items of a user - take rc_bucket_add_few instead.
__device__ __forceinline__ void rc_bucket_add(int *bucket, bool on, int g) {
    const int lane = threadIdx.x % kWave;
    unsigned long long open = __ballot(on);
    for (int it = 0; it < kRcAgg && open; ++it) {           // (uniform over the wave)
        const int leader = __ffsll((long long)open) - 1;
        const int gl = __shfl(g, leader, kWave);
        const unsigned long long same = __ballot(on && g == gl);
        if (lane == leader) atomicAdd(&bucket[gl], __popcll(same));
        open &= ~same;
    }
    if ((open >> lane) & 1ull) atomicAdd(&bucket[g], 1);
}

// The same additions for a block of c < kRcFew targets and NX items per lane: one ballot and popcount per (bucket, item) -
// scalar work, no cross-lane traffic - and lane k adds bucket k's count of the whole wave with one atomic, if it is not 0.
template <int NX>
__device__ __forceinline__ void rc_bucket_add_few(int *bucket, const bool (&on)[NX], const int (&g)[NX], int c) {
    const int lane = threadIdx.x % kWave;
    int mine = 0;
    for (int k = 0; k <= c; ++k) {                          // (uniform)
        int tot = 0;
#pragma unroll
        for (int x = 0; x < NX; ++x) tot += __popcll(__ballot(on[x] && g[x] == k));
        if (lane == k) mine = tot;
    }
    if (mine) atomicAdd(&bucket[lane], mine);               // (lane <= c: only those lanes got a count)
}

// Called by every thread after the last bucket addition: bucket[r] becomes the position of sorted target r < c; returns
// the buckets' total, the number of eligible items.  Ends with a barrier.
template <class Ent>
__device__ __forceinline__ int rc_positions(RcState<Ent> &st, int c) {
    const int tid = threadIdx.x;
    __syncthreads();
    const int b0 = 2 * tid <= c ? st.bucket[2 * tid] : 0, b1 = 2 * tid + 1 <= c ? st.bucket[2 * tid + 1] : 0;
    st.scan[tid] = b0 + b1;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {
        const int add = tid >= off ? st.scan[tid - off] : 0;
        __syncthreads();
        st.scan[tid] += add;
        __syncthreads();
    }
    const int incl = st.scan[tid];
    const int total = st.scan[kBlock - 1] + (c == kRcTc ? st.bucket[kRcTc] : 0);
    __syncthreads();
    if (2 * tid < c) st.bucket[2 * tid] = incl - b1 - 1;
    if (2 * tid + 1 < c) st.bucket[2 * tid + 1] = incl - 1;
    __syncthreads();
    return total;
}

}  // namespace daisy
