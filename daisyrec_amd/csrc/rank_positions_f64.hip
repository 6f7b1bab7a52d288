// Exact ranks of held-out items over all items for the models that score by a fixed-order fp64 sum (DESIGN.md section
// 28): EASE, SLiM, ItemKNN / UserKNN and PureSVD.  One launch, one workgroup per request: the scorers of
// rank_f64_scorers.h in front (the structs rank_full_f64.hip ranks with, so a target's score and an item's score are the
// list's bits), the counting body of rank_f64_positions.h behind.  Nothing of size [users, items] is written or allocated,
// there is no workspace, and the counts are integer LDS atomics: two runs give the same bits.
#include <limits.h>

#include "common.h"
#include "rank_f64_positions.h"
#include "rank_f64_scorers.h"

namespace daisy {
namespace {

constexpr int kHwLdsBytes = 160 * 1024;            // LDS of a CDNA4 compute unit
static_assert(kSparseDotLdsItems * (int)sizeof(float) + kRpLdsBytes <= kHwLdsBytes,
              "the user's dense row and the target block share the LDS");

// what every kernel gets besides its model: the requests, the exclusion, the targets and the outputs
struct RpArgs {
    const int64_t *__restrict__ users;
    const int64_t *__restrict__ indptr;
    const int32_t *__restrict__ eitems;
    const int64_t *__restrict__ t_indptr;
    const int32_t *__restrict__ t_items;
    const int64_t *__restrict__ out_indptr;
    int64_t n_targets;
    int32_t *__restrict__ out_pos;
    void *__restrict__ out_scores;
    int32_t *__restrict__ out_eligible;
};

template <class Scorer, class OutT>
__device__ __forceinline__ void rp_request(const Scorer &sc, int64_t I, const RpArgs &a, int64_t b, int64_t u, bool valid) {
    int64_t lo, hi;
    excl_row(a.indptr, valid, u, lo, hi);
    const int64_t t_lo = valid ? a.t_indptr[u] : 0, t_hi = valid ? a.t_indptr[u + 1] : 0;
    const int64_t dst0 = a.out_indptr[b];
    int64_t t_len = a.out_indptr[b + 1] - dst0;             // the caller's row length, never more than the target row's
    if (t_len > t_hi - t_lo) t_len = t_hi - t_lo;
    rank_f64_positions_body(sc, I, a.eitems, lo, hi, a.t_items, t_lo, t_len, dst0, a.n_targets, a.out_pos,
                            static_cast<OutT *>(a.out_scores), a.out_eligible ? a.out_eligible + b : nullptr);
}

__global__ __launch_bounds__(kBlock) void k_ease_full_rank_positions(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const double *__restrict__ W, int64_t U, int64_t I, RpArgs a) {
    const int64_t b = blockIdx.x;
    const int64_t u = a.users[b];
    const bool valid = u >= 0 && u < U;
    const EaseScorer sc{col, val, valid ? row_ptr[u] : 0, valid ? row_ptr[u + 1] : 0, W, I};
    rp_request<EaseScorer, double>(sc, I, a, b, u, valid);
}

template <bool LDS, bool ROUND32, class OutT>
__global__ __launch_bounds__(kBlock) void k_sparse_full_rank_positions(
    const int64_t *__restrict__ l_ptr, const int32_t *__restrict__ l_col, const float *__restrict__ l_val, int64_t n_rows,
    int64_t inner, const int64_t *__restrict__ r_ptr, const int32_t *__restrict__ r_row, const float *__restrict__ r_val,
    int64_t n_cols, RpArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rp_x[];
    const int64_t b = blockIdx.x;
    const int64_t u = a.users[b];
    const bool valid = u >= 0 && u < n_rows;
    const int64_t beg = valid ? l_ptr[u] : 0, end = valid ? l_ptr[u + 1] : 0;
    if (LDS) sparse_row_to_lds(rp_x, inner, l_col, l_val, beg, end);
    const SparseDotScorer<LDS, ROUND32> sc{rp_x, l_col, l_val, beg, end, inner, r_ptr, r_row, r_val, valid};
    rp_request<SparseDotScorer<LDS, ROUND32>, OutT>(sc, n_cols, a, b, u, valid);
}

__global__ __launch_bounds__(kBlock) void k_psvd_full_rank_positions(const double *__restrict__ user_vec,
                                                                     const double *__restrict__ item_vec, int64_t U,
                                                                     int64_t I, int k, RpArgs a) {
    const int64_t b = blockIdx.x;
    const int64_t u = a.users[b];
    const bool valid = u >= 0 && u < U;
    const PsvdScorer sc{user_vec + (valid ? u : 0) * k, item_vec, k, valid};
    rp_request<PsvdScorer, double>(sc, I, a, b, u, valid);
}

// the checks every entry shares; `what` is the entry's name
int rp_check(const char *what, int64_t user_num, int64_t item_num, int64_t n, int64_t n_targets, const RpArgs &a) {
    DAISY_CHECK_ARG(user_num >= 1 && item_num >= 1 && item_num <= INT_MAX, "%s: user_num=%lld item_num=%lld (item_num in [1, 2^31))",
                    what, (long long)user_num, (long long)item_num);
    DAISY_CHECK_ARG(n >= 0 && n <= INT_MAX, "%s: bad request count n=%lld", what, (long long)n);
    DAISY_CHECK_ARG(n_targets >= 0, "%s: bad target count n_targets=%lld", what, (long long)n_targets);
    DAISY_CHECK_ARG(n == 0 || (a.users && a.t_indptr && a.out_indptr), "%s: NULL argument (users, tgt_indptr, out_indptr)", what);
    DAISY_CHECK_ARG(n == 0 || n_targets == 0 || (a.t_items && a.out_pos), "%s: NULL argument (tgt_items, out_pos)", what);
    DAISY_CHECK_ARG((a.indptr != nullptr) == (a.eitems != nullptr),
                    "%s: excl_indptr and excl_items are given together or not at all", what);
    return DAISY_OK;
}

// nothing to launch: no request, or neither a target nor an eligible count to write
bool rp_empty(int64_t n, const RpArgs &a) { return n == 0 || (a.n_targets == 0 && !a.out_eligible); }

template <bool ROUND32, class OutT>
int sparse_full_rank_positions(const char *what, const int64_t *l_ptr, const int32_t *l_col, const float *l_val, int64_t n_rows,
                               int64_t inner, const int64_t *r_ptr, const int32_t *r_row, const float *r_val, int64_t n_cols,
                               int64_t n, const RpArgs &a, int32_t path, daisy_stream_t stream) {
    DAISY_CHECK_ARG(l_ptr && l_col && l_val && r_ptr && r_row && r_val, "%s: NULL argument", what);
    if (const int rc = rp_check(what, n_rows, n_cols, n, a.n_targets, a)) return rc;
    DAISY_CHECK_ARG(inner >= 1 && inner <= INT_MAX, "%s: inner=%lld outside [1, 2^31)", what, (long long)inner);
    DAISY_CHECK_ARG(path >= DAISY_SLIM_PATH_AUTO && path <= DAISY_SLIM_PATH_GLOBAL, "%s: path=%d", what, path);
    const bool lds = path == DAISY_SLIM_PATH_LDS || (path == DAISY_SLIM_PATH_AUTO && inner <= kSparseDotLdsItems);
    DAISY_CHECK_ARG(!lds || inner <= kSparseDotLdsItems, "%s: the LDS path holds at most %d entries (inner=%lld)", what,
                    kSparseDotLdsItems, (long long)inner);
    if (rp_empty(n, a)) return DAISY_OK;
    hipStream_t s = as_stream(stream);
    if (lds) {
        auto kern = k_sparse_full_rank_positions<true, ROUND32, OutT>;
        DAISY_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      kSparseDotLdsItems * (int)sizeof(float)));
        hipLaunchKernelGGL(kern, dim3((unsigned)n), dim3(kBlock), (size_t)inner * sizeof(float), s, l_ptr, l_col, l_val, n_rows,
                           inner, r_ptr, r_row, r_val, n_cols, a);
    } else {
        hipLaunchKernelGGL((k_sparse_full_rank_positions<false, ROUND32, OutT>), dim3((unsigned)n), dim3(kBlock), 0, s, l_ptr,
                           l_col, l_val, n_rows, inner, r_ptr, r_row, r_val, n_cols, a);
    }
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // namespace
}  // namespace daisy

using namespace daisy;

extern "C" {

int daisy_ease_full_rank_positions(const int64_t *row_ptr, const int32_t *col, const float *val, const double *W,
                                   int64_t user_num, int64_t item_num, const int64_t *users, int64_t n,
                                   const int64_t *excl_indptr, const int32_t *excl_items, const int64_t *tgt_indptr,
                                   const int32_t *tgt_items, const int64_t *out_indptr, int64_t n_targets, int32_t *out_pos,
                                   double *out_scores, int32_t *out_eligible, daisy_stream_t stream) {
    const char *what = "ease_full_rank_positions";
    const RpArgs a{users, excl_indptr, excl_items, tgt_indptr, tgt_items, out_indptr, n_targets, out_pos, out_scores, out_eligible};
    DAISY_CHECK_ARG(row_ptr && col && val && W, "%s: NULL argument", what);
    if (const int rc = rp_check(what, user_num, item_num, n, n_targets, a)) return rc;
    if (rp_empty(n, a)) return DAISY_OK;
    hipLaunchKernelGGL(k_ease_full_rank_positions, dim3((unsigned)n), dim3(kBlock), 0, as_stream(stream), row_ptr, col, val, W,
                       user_num, item_num, a);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_slim_full_rank_positions(const int64_t *row_ptr, const int32_t *col, const float *val, int64_t user_num,
                                   int64_t item_num, const int64_t *w_ptr, const int32_t *w_row, const float *w_val,
                                   const int64_t *users, int64_t n, const int64_t *excl_indptr, const int32_t *excl_items,
                                   const int64_t *tgt_indptr, const int32_t *tgt_items, const int64_t *out_indptr,
                                   int64_t n_targets, int32_t *out_pos, float *out_scores, int32_t *out_eligible, int32_t path,
                                   daisy_stream_t stream) {
    const RpArgs a{users, excl_indptr, excl_items, tgt_indptr, tgt_items, out_indptr, n_targets, out_pos, out_scores, out_eligible};
    return sparse_full_rank_positions<true, float>("slim_full_rank_positions", row_ptr, col, val, user_num, item_num, w_ptr, w_row,
                                                   w_val, item_num, n, a, path, stream);
}

int daisy_knn_full_rank_positions(const int64_t *l_ptr, const int32_t *l_col, const float *l_val, int64_t n_rows, int64_t inner,
                                  const int64_t *r_ptr, const int32_t *r_row, const float *r_val, int64_t n_cols,
                                  const int64_t *users, int64_t n, const int64_t *excl_indptr, const int32_t *excl_items,
                                  const int64_t *tgt_indptr, const int32_t *tgt_items, const int64_t *out_indptr,
                                  int64_t n_targets, int32_t *out_pos, double *out_scores, int32_t *out_eligible, int32_t path,
                                  daisy_stream_t stream) {
    const RpArgs a{users, excl_indptr, excl_items, tgt_indptr, tgt_items, out_indptr, n_targets, out_pos, out_scores, out_eligible};
    return sparse_full_rank_positions<false, double>("knn_full_rank_positions", l_ptr, l_col, l_val, n_rows, inner, r_ptr, r_row,
                                                     r_val, n_cols, n, a, path, stream);
}

int daisy_psvd_full_rank_positions(const double *user_vec, const double *item_vec, int64_t user_num, int64_t item_num, int32_t k,
                                   const int64_t *users, int64_t n, const int64_t *excl_indptr, const int32_t *excl_items,
                                   const int64_t *tgt_indptr, const int32_t *tgt_items, const int64_t *out_indptr,
                                   int64_t n_targets, int32_t *out_pos, double *out_scores, int32_t *out_eligible,
                                   daisy_stream_t stream) {
    const char *what = "psvd_full_rank_positions";
    const RpArgs a{users, excl_indptr, excl_items, tgt_indptr, tgt_items, out_indptr, n_targets, out_pos, out_scores, out_eligible};
    DAISY_CHECK_ARG(user_vec && item_vec, "%s: NULL argument", what);
    DAISY_CHECK_ARG(k >= 1 && k <= DAISY_PSVD_MAX_C, "%s: k=%d factors outside [1, %d]", what, k, DAISY_PSVD_MAX_C);
    if (const int rc = rp_check(what, user_num, item_num, n, n_targets, a)) return rc;
    if (rp_empty(n, a)) return DAISY_OK;
    hipLaunchKernelGGL(k_psvd_full_rank_positions, dim3((unsigned)n), dim3(kBlock), 0, as_stream(stream), user_vec, item_vec,
                       user_num, item_num, (int)k, a);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // extern "C"
