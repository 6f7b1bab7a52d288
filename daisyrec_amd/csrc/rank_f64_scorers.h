// The scorers of the full rankings on fixed-order fp64 sums (DESIGN.md sections 25 and 28): one struct per model family
// around the score expressions of score_f64.h, shared by rank_full_f64.hip (the lists) and rank_positions_f64.hip (the
// exact positions), so that a score is one function call whichever kernel asks for it - and so its bits.
#pragma once

#include "common.h"
#include "score_f64.h"

namespace daisy {

struct EaseScorer {
    const int32_t *__restrict__ col;
    const float *__restrict__ val;
    int64_t beg, end;
    const double *__restrict__ W;
    int64_t I;
    __device__ __forceinline__ double score(int64_t it) const { return ease_score(col, val, beg, end, W, I, it); }
};

// ROUND32: SLiM ranks on the score after its rounding to fp32
template <bool LDS, bool ROUND32>
struct SparseDotScorer {
    const float *x;
    const int32_t *__restrict__ l_col;
    const float *__restrict__ l_val;
    int64_t beg, end, inner;
    const int64_t *__restrict__ r_ptr;
    const int32_t *__restrict__ r_row;
    const float *__restrict__ r_val;
    bool valid;
    __device__ __forceinline__ double score(int64_t it) const {
        const double s = valid ? sparse_dot_score<LDS>(x, l_col, l_val, beg, end, inner, r_ptr, r_row, r_val, it) : 0.0;
        return ROUND32 ? (double)(float)s : s;
    }
};

struct PsvdScorer {
    const double *__restrict__ uv;
    const double *__restrict__ item_vec;
    int k;
    bool valid;
    __device__ __forceinline__ double score(int64_t it) const { return valid ? psvd_score(uv, item_vec + it * k, k) : 0.0; }
};

// the user's row of the exclusion CSR (an id outside [0, U): an empty row)
__device__ __forceinline__ void excl_row(const int64_t *__restrict__ indptr, bool valid, int64_t u, int64_t &lo, int64_t &hi) {
    lo = hi = 0;
    if (indptr && valid) { lo = indptr[u]; hi = indptr[u + 1]; }
}

}  // namespace daisy
