// MostPop (daisy/model/PopRecommender.py): the item counts by integer atomics (their sum does not depend on
// the order), score = cnt / (1 + cnt) as the reference's one fp64 division, and the ranking of gathered scores by the
// shared fp64 top-k (score descending, ties to the lower candidate position).  No floating-point atomics.
#include <limits.h>

#include "common.h"
#include "topk_f64.h"

namespace daisy {
namespace {

__global__ __launch_bounds__(kBlock) void k_pop_count(const void *__restrict__ items, int is_i64, int64_t nnz,
                                                      int64_t item_num, unsigned long long *__restrict__ cnt) {
    for (int64_t e = blockIdx.x * (int64_t)kBlock + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kBlock) {
        const int64_t it = is_i64 ? static_cast<const int64_t *>(items)[e] : (int64_t) static_cast<const int32_t *>(items)[e];
        if (it >= 0 && it < item_num) atomicAdd(&cnt[it], 1ull);
    }
}

// PopRecommender.py:33: item_cnt_ref / (1 + item_cnt_ref) on float64 counts
__global__ __launch_bounds__(kBlock) void k_pop_score(const int64_t *__restrict__ cnt, int64_t item_num,
                                                      double *__restrict__ score) {
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < item_num; i += (int64_t)gridDim.x * kBlock) {
        const double c = (double)cnt[i];
        score[i] = c / (1.0 + c);
    }
}

// One workgroup per row of candidates: gather, then the top-k.  items == NULL: the row is the score table itself.
__global__ __launch_bounds__(kBlock) void k_pop_rank(const double *__restrict__ score, int64_t item_num,
                                                     const int64_t *__restrict__ items, int64_t C, int topk, double *gathered,
                                                     int64_t *__restrict__ out_ids) {
    const int64_t b = blockIdx.x;
    if (!items) {
        topk_f64_select(score, C, topk, nullptr, out_ids + b * topk);
        return;
    }
    double *row = gathered + b * C;
    for (int64_t c = threadIdx.x; c < C; c += kBlock) {
        const int64_t it = items[b * C + c];
        row[c] = (it >= 0 && it < item_num) ? score[it] : 0.0;
    }
    topk_f64_select(row, C, topk, items + b * C, out_ids + b * topk);
}

}  // namespace
}  // namespace daisy

using namespace daisy;

extern "C" {

int daisy_pop_fit(const void *items, int32_t items_is_i64, int64_t nnz, int64_t item_num, int64_t *cnt, double *score,
                  daisy_stream_t stream) {
    DAISY_CHECK_ARG(cnt && score && (items || nnz == 0), "pop_fit: NULL argument");
    DAISY_CHECK_ARG(nnz >= 0 && item_num >= 1 && item_num <= INT_MAX, "pop_fit: nnz=%lld item_num=%lld", (long long)nnz,
                    (long long)item_num);
    hipStream_t s = as_stream(stream);
    DAISY_HIP(hipMemsetAsync(cnt, 0, (size_t)item_num * sizeof(int64_t), s));
    if (nnz > 0) {
        hipLaunchKernelGGL(k_pop_count, dim3(grid_for(nnz, kBlock)), dim3(kBlock), 0, s, items, (int)(items_is_i64 != 0), nnz,
                           item_num, reinterpret_cast<unsigned long long *>(cnt));
        DAISY_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_pop_score, dim3(grid_for(item_num, kBlock)), dim3(kBlock), 0, s, cnt, item_num, score);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_pop_rank(const double *score, int64_t item_num, const int64_t *items, int64_t B, int64_t C, int32_t topk,
                   double *gathered, int64_t *out_ids, daisy_stream_t stream) {
    DAISY_CHECK_ARG(score && out_ids && (gathered || !items), "pop_rank: NULL argument");
    DAISY_CHECK_ARG(item_num >= 1 && item_num <= INT_MAX && B >= 0 && B <= INT_MAX, "pop_rank: item_num=%lld B=%lld",
                    (long long)item_num, (long long)B);
    DAISY_CHECK_ARG(items ? C >= 1 : (C == item_num && B <= 1),
                    "pop_rank: C=%lld candidates per row (item_num and one row when items == NULL)", (long long)C);
    DAISY_CHECK_ARG(topk >= 1 && topk <= C, "pop_rank: topk=%d outside [1, C=%lld]", topk, (long long)C);
    if (B == 0) return DAISY_OK;
    hipLaunchKernelGGL(k_pop_rank, dim3((unsigned)B), dim3(kBlock), 0, as_stream(stream), score, item_num, items, C, (int)topk,
                       gathered, out_ids);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // extern "C"
