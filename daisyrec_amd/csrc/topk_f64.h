// The top-k of one row of fp64 scores, shared by the models that rank on fp64 keys (puresvd.hip, ease.hip).
#pragma once

#include <limits.h>

#include "common.h"

namespace daisy {

// Called by every thread of a kBlock workgroup after it has written its part of row[C] (the barrier is in here): topk
// rounds of "the largest score after the previous pick" in the order (score descending, position ascending), compared as
// fp64.  out_row[sel] = ids_row[position] (the position itself when ids_row == NULL); when nothing comparable is left
// (NaN scores) the rest of out_row is filled with -1.
__device__ __forceinline__ void topk_f64_select(const double *row, int64_t C, int topk, const int64_t *__restrict__ ids_row,
                                                int64_t *__restrict__ out_row) {
    __shared__ double s_v[kBlock / kWave];
    __shared__ long long s_i[kBlock / kWave];
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    __syncthreads();
    double pv = 0.0;
    long long pp = -1;                  // the previous pick; pp < 0: none yet
    for (int sel = 0; sel < topk; ++sel) {
        double bv = 0.0;
        long long bi = LLONG_MAX;
        for (int64_t cidx = tid; cidx < C; cidx += kBlock) {           // ascending position: the first maximum is the lowest
            const double v = row[cidx];
            const bool elig = (pp < 0) ? (v == v) : (v < pv || (v == pv && cidx > pp));
            if (elig && (bi == LLONG_MAX || v > bv)) { bv = v; bi = cidx; }
        }
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {
            const double ov = __shfl_xor(bv, off, kWave);
            const long long oi = __shfl_xor(bi, off, kWave);
            if (oi != LLONG_MAX && (bi == LLONG_MAX || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
        }
        if (lane == 0) { s_v[wave] = bv; s_i[wave] = bi; }
        __syncthreads();
        bv = s_v[0];
        bi = s_i[0];
#pragma unroll
        for (int wv = 1; wv < kBlock / kWave; ++wv) {
            const double ov = s_v[wv];
            const long long oi = s_i[wv];
            if (oi != LLONG_MAX && (bi == LLONG_MAX || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
        }
        __syncthreads();
        if (bi == LLONG_MAX) {                                        // nothing comparable left
            for (int t = sel + tid; t < topk; t += kBlock) out_row[t] = -1;
            return;
        }
        if (tid == 0) out_row[sel] = ids_row ? ids_row[bi] : (int64_t)bi;
        pv = bv;
        pp = bi;
    }
}

}  // namespace daisy
