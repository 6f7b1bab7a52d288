// Full ranking of many users for the models that score by a fixed-order fp64 sum: EASE, SLiM,
// ItemKNN / UserKNN and PureSVD.  One workgroup per requested user: the front half is the model's own score expression
// (score_f64.h - the very functions k_ease_rank, k_slim_scores, k_knn_rank and k_psvd_rank call, so the scores agree bit
// for bit), the back half the streaming selector of rank_f64_users.h, which masks the user's exclusion row and keeps or
// drops a score while it is still in a register.  Nothing of size [users, items] is written or allocated.
#include <limits.h>

#include "common.h"
#include "rank_f64_scorers.h"
#include "rank_f64_users.h"

namespace daisy {
namespace {

constexpr int kHwLdsBytes = 160 * 1024;            // LDS of a CDNA4 compute unit
static_assert(kSparseDotLdsItems * (int)sizeof(float) + kRfLdsBytes <= kHwLdsBytes,
              "the user's dense row and the candidate buffer share the LDS");

__global__ __launch_bounds__(kBlock) void k_ease_full_rank_users(
    const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const double *__restrict__ W, int64_t U, int64_t I, const int64_t *__restrict__ users,
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ eitems, int topk, int64_t *__restrict__ out_ids,
    double *__restrict__ out_scores) {
    const int64_t b = blockIdx.x;
    const int64_t u = users[b];
    const bool valid = u >= 0 && u < U;
    const EaseScorer sc{col, val, valid ? row_ptr[u] : 0, valid ? row_ptr[u + 1] : 0, W, I};
    int64_t lo, hi;
    excl_row(indptr, valid, u, lo, hi);
    rank_f64_users_body(sc, I, eitems, lo, hi, topk, out_ids + b * topk, out_scores ? out_scores + b * topk : nullptr);
}

template <bool LDS, bool ROUND32, class OutT>
__global__ __launch_bounds__(kBlock) void k_sparse_full_rank_users(
    const int64_t *__restrict__ l_ptr, const int32_t *__restrict__ l_col, const float *__restrict__ l_val, int64_t n_rows,
    int64_t inner, const int64_t *__restrict__ r_ptr, const int32_t *__restrict__ r_row, const float *__restrict__ r_val,
    int64_t n_cols, const int64_t *__restrict__ users, const int64_t *__restrict__ indptr,
    const int32_t *__restrict__ eitems, int topk, int64_t *__restrict__ out_ids, OutT *__restrict__ out_scores) {
    extern __shared__ __attribute__((aligned(16))) float rf_x[];
    const int64_t b = blockIdx.x;
    const int64_t u = users[b];
    const bool valid = u >= 0 && u < n_rows;
    const int64_t beg = valid ? l_ptr[u] : 0, end = valid ? l_ptr[u + 1] : 0;
    if (LDS) sparse_row_to_lds(rf_x, inner, l_col, l_val, beg, end);
    const SparseDotScorer<LDS, ROUND32> sc{rf_x, l_col, l_val, beg, end, inner, r_ptr, r_row, r_val, valid};
    int64_t lo, hi;
    excl_row(indptr, valid, u, lo, hi);
    rank_f64_users_body(sc, n_cols, eitems, lo, hi, topk, out_ids + b * topk, out_scores ? out_scores + b * topk : nullptr);
}

__global__ __launch_bounds__(kBlock) void k_psvd_full_rank_users(
    const double *__restrict__ user_vec, const double *__restrict__ item_vec, int64_t U, int64_t I, int k,
    const int64_t *__restrict__ users, const int64_t *__restrict__ indptr, const int32_t *__restrict__ eitems, int topk,
    int64_t *__restrict__ out_ids, double *__restrict__ out_scores) {
    const int64_t b = blockIdx.x;
    const int64_t u = users[b];
    const bool valid = u >= 0 && u < U;
    const PsvdScorer sc{user_vec + (valid ? u : 0) * k, item_vec, k, valid};
    int64_t lo, hi;
    excl_row(indptr, valid, u, lo, hi);
    rank_f64_users_body(sc, I, eitems, lo, hi, topk, out_ids + b * topk, out_scores ? out_scores + b * topk : nullptr);
}

// the checks every entry shares; `what` is the entry's name
int rf_check(const char *what, int64_t user_num, int64_t item_num, const int64_t *users, int64_t n,
             const int64_t *excl_indptr, const int32_t *excl_items, int32_t topk, const int64_t *out_ids) {
    DAISY_CHECK_ARG(user_num >= 1 && item_num >= 1 && item_num <= INT_MAX, "%s: user_num=%lld item_num=%lld (item_num in [1, 2^31))",
                    what, (long long)user_num, (long long)item_num);
    DAISY_CHECK_ARG(n >= 0 && n <= INT_MAX, "%s: bad user count n=%lld", what, (long long)n);
    DAISY_CHECK_ARG(n == 0 || (users && out_ids), "%s: NULL argument (users, out_ids)", what);
    DAISY_CHECK_ARG((excl_indptr != nullptr) == (excl_items != nullptr),
                    "%s: excl_indptr and excl_items are given together or not at all", what);
    DAISY_CHECK_ARG(topk <= kRfTopkCap, "%s: topk=%d above the cap of %d (the candidate buffer lives in LDS)", what, topk,
                    kRfTopkCap);
    DAISY_CHECK_ARG(topk >= 1, "%s: topk=%d must be >= 1", what, topk);
    return DAISY_OK;
}

template <bool ROUND32, class OutT>
int sparse_full_rank_users(const char *what, const int64_t *l_ptr, const int32_t *l_col, const float *l_val, int64_t n_rows,
                           int64_t inner, const int64_t *r_ptr, const int32_t *r_row, const float *r_val, int64_t n_cols,
                           const int64_t *users, int64_t n, const int64_t *excl_indptr, const int32_t *excl_items,
                           int32_t topk, int64_t *out_ids, OutT *out_scores, int32_t path, daisy_stream_t stream) {
    DAISY_CHECK_ARG(l_ptr && l_col && l_val && r_ptr && r_row && r_val, "%s: NULL argument", what);
    if (const int rc = rf_check(what, n_rows, n_cols, users, n, excl_indptr, excl_items, topk, out_ids)) return rc;
    DAISY_CHECK_ARG(inner >= 1 && inner <= INT_MAX, "%s: inner=%lld outside [1, 2^31)", what, (long long)inner);
    DAISY_CHECK_ARG(path >= DAISY_SLIM_PATH_AUTO && path <= DAISY_SLIM_PATH_GLOBAL, "%s: path=%d", what, path);
    const bool lds = path == DAISY_SLIM_PATH_LDS || (path == DAISY_SLIM_PATH_AUTO && inner <= kSparseDotLdsItems);
    DAISY_CHECK_ARG(!lds || inner <= kSparseDotLdsItems, "%s: the LDS path holds at most %d entries (inner=%lld)", what,
                    kSparseDotLdsItems, (long long)inner);
    if (n == 0) return DAISY_OK;
    hipStream_t s = as_stream(stream);
    if (lds) {
        auto kern = k_sparse_full_rank_users<true, ROUND32, OutT>;
        DAISY_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      kSparseDotLdsItems * (int)sizeof(float)));
        hipLaunchKernelGGL(kern, dim3((unsigned)n), dim3(kBlock), (size_t)inner * sizeof(float), s, l_ptr, l_col, l_val, n_rows,
                           inner, r_ptr, r_row, r_val, n_cols, users, excl_indptr, excl_items, (int)topk, out_ids, out_scores);
    } else {
        hipLaunchKernelGGL((k_sparse_full_rank_users<false, ROUND32, OutT>), dim3((unsigned)n), dim3(kBlock), 0, s, l_ptr, l_col,
                           l_val, n_rows, inner, r_ptr, r_row, r_val, n_cols, users, excl_indptr, excl_items, (int)topk, out_ids,
                           out_scores);
    }
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // namespace
}  // namespace daisy

using namespace daisy;

extern "C" {

size_t daisy_rank_f64_users_workspace_bytes(int64_t n, int64_t item_num, int32_t topk) {
    (void)n; (void)item_num; (void)topk;
    return 0;                                   // the candidates of a user live in LDS; nothing of size n * item_num exists
}

int daisy_ease_full_rank_users(const int64_t *row_ptr, const int32_t *col, const float *val, const double *W, int64_t user_num,
                               int64_t item_num, const int64_t *users, int64_t n, const int64_t *excl_indptr,
                               const int32_t *excl_items, int32_t topk, int64_t *out_ids, double *out_scores,
                               daisy_stream_t stream) {
    const char *what = "ease_full_rank_users";
    DAISY_CHECK_ARG(row_ptr && col && val && W, "%s: NULL argument", what);
    if (const int rc = rf_check(what, user_num, item_num, users, n, excl_indptr, excl_items, topk, out_ids)) return rc;
    if (n == 0) return DAISY_OK;
    hipLaunchKernelGGL(k_ease_full_rank_users, dim3((unsigned)n), dim3(kBlock), 0, as_stream(stream), row_ptr, col, val, W,
                       user_num, item_num, users, excl_indptr, excl_items, (int)topk, out_ids, out_scores);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_slim_full_rank_users(const int64_t *row_ptr, const int32_t *col, const float *val, int64_t user_num, int64_t item_num,
                               const int64_t *w_ptr, const int32_t *w_row, const float *w_val, const int64_t *users, int64_t n,
                               const int64_t *excl_indptr, const int32_t *excl_items, int32_t topk, int64_t *out_ids,
                               float *out_scores, int32_t path, daisy_stream_t stream) {
    return sparse_full_rank_users<true, float>("slim_full_rank_users", row_ptr, col, val, user_num, item_num, w_ptr, w_row, w_val,
                                               item_num, users, n, excl_indptr, excl_items, topk, out_ids, out_scores, path,
                                               stream);
}

int daisy_knn_full_rank_users(const int64_t *l_ptr, const int32_t *l_col, const float *l_val, int64_t n_rows, int64_t inner,
                              const int64_t *r_ptr, const int32_t *r_row, const float *r_val, int64_t n_cols,
                              const int64_t *users, int64_t n, const int64_t *excl_indptr, const int32_t *excl_items,
                              int32_t topk, int64_t *out_ids, double *out_scores, int32_t path, daisy_stream_t stream) {
    return sparse_full_rank_users<false, double>("knn_full_rank_users", l_ptr, l_col, l_val, n_rows, inner, r_ptr, r_row, r_val,
                                                 n_cols, users, n, excl_indptr, excl_items, topk, out_ids, out_scores, path,
                                                 stream);
}

int daisy_psvd_full_rank_users(const double *user_vec, const double *item_vec, int64_t user_num, int64_t item_num, int32_t k,
                               const int64_t *users, int64_t n, const int64_t *excl_indptr, const int32_t *excl_items,
                               int32_t topk, int64_t *out_ids, double *out_scores, daisy_stream_t stream) {
    const char *what = "psvd_full_rank_users";
    DAISY_CHECK_ARG(user_vec && item_vec, "%s: NULL argument", what);
    DAISY_CHECK_ARG(k >= 1 && k <= DAISY_PSVD_MAX_C, "%s: k=%d factors outside [1, %d]", what, k, DAISY_PSVD_MAX_C);
    if (const int rc = rf_check(what, user_num, item_num, users, n, excl_indptr, excl_items, topk, out_ids)) return rc;
    if (n == 0) return DAISY_OK;
    hipLaunchKernelGGL(k_psvd_full_rank_users, dim3((unsigned)n), dim3(kBlock), 0, as_stream(stream), user_vec, item_vec,
                       user_num, item_num, (int)k, users, excl_indptr, excl_items, (int)topk, out_ids, out_scores);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // extern "C"
