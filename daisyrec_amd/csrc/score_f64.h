// The per-candidate score expressions of the models that rank on fixed-order fp64 sums (ease.hip, slim.hip, knn.hip,
// puresvd.hip), shared with the streaming full ranking of rank_full_f64.hip: one definition per
// expression, so the kernels that call it agree bit for bit.  A score depends on (user, item) alone.
#pragma once

#include "common.h"

namespace daisy {

constexpr int kSparseDotLdsItems = 32768;          // a user's dense fp32 row in LDS: 128 KB (slim_scores, knn_rank)

// value at column r of a CSR row [beg, end) whose columns ascend; 0 when the row has no such entry.  The search is
// bounded by the row's length whatever the row holds.
__device__ __forceinline__ float sparse_row_lookup(const int32_t *__restrict__ col, const float *__restrict__ val,
                                                   int64_t beg, int64_t end, int32_t r) {
    while (beg < end) {                                 // columns ascend within a row
        const int64_t mid = beg + (end - beg) / 2;
        const int32_t c = col[mid];
        if (c == r) return val[mid];
        if (c < r) beg = mid + 1; else end = mid;
    }
    return 0.f;
}

// Called by every thread of the workgroup: x[0 .. inner) = the CSR row [beg, end) as a dense vector (the last write of a
// column stays).  Ends with a barrier.
__device__ __forceinline__ void sparse_row_to_lds(float *x, int64_t inner, const int32_t *__restrict__ col,
                                                  const float *__restrict__ val, int64_t beg, int64_t end) {
    for (int64_t i = threadIdx.x; i < inner; i += kBlock) x[i] = 0.f;
    __syncthreads();
    for (int64_t e = beg + threadIdx.x; e < end; e += kBlock) {
        const int32_t c = col[e];
        if (c >= 0 && c < inner) x[c] = val[e];
    }
    __syncthreads();
}

// SLiM's and the neighbourhood models' score before any rounding: the sum over the entries [r_ptr[it], r_ptr[it + 1]) of
// column `it` of the right operand, in stored (ascending row) order, of (double) x[row] * (double) value; x is the
// user's row of the left operand, dense in LDS (LDS) or looked up in its CSR row [beg, end).  The product of two fp32
// values is exact in fp64.
template <bool LDS>
__device__ __forceinline__ double sparse_dot_score(const float *x, const int32_t *__restrict__ l_col,
                                                   const float *__restrict__ l_val, int64_t beg, int64_t end, int64_t inner,
                                                   const int64_t *__restrict__ r_ptr, const int32_t *__restrict__ r_row,
                                                   const float *__restrict__ r_val, int64_t it) {
    double s = 0.0;
    const int64_t pe = r_ptr[it + 1];
    for (int64_t e = r_ptr[it]; e < pe; ++e) {             // ascending row: the order of the fp64 sum
        const int32_t k = r_row[e];
        if (k < 0 || k >= inner) continue;
        const float xv = LDS ? x[k] : sparse_row_lookup(l_col, l_val, beg, end, k);
        s += (double)xv * (double)r_val[e];
    }
    return s;
}

// EASE: X[u, :] W[:, it] over the user's CSR entries [beg, end) in stored order
__device__ __forceinline__ double ease_score(const int32_t *__restrict__ col, const float *__restrict__ val, int64_t beg,
                                             int64_t end, const double *__restrict__ W, int64_t I, int64_t it) {
    double s = 0.0;
    for (int64_t e = beg; e < end; ++e) {
        const int64_t r = col[e];
        if (r >= 0 && r < I) s = fma((double)val[e], W[r * I + it], s);
    }
    return s;
}

// PureSVD: <uv, iv> over the k factors in ascending order
__device__ __forceinline__ double psvd_score(const double *__restrict__ uv, const double *__restrict__ iv, int k) {
    double s = 0.0;
    for (int f = 0; f < k; ++f) s = fma(uv[f], iv[f], s);
    return s;
}

}  // namespace daisy
