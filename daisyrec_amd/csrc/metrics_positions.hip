// The per-list KPIs of daisy_ranking_kpis (metrics.hip) from the exact rank positions of the held-out
// items (rank_positions.hip) instead of from ranked lists: the reference's list definitions applied
// to the implied list of length K, at any K.  One wave per request, 64 consecutive requests per wave.  A chunk of 64
// positions of the row is staged in LDS with the rank of each among the row's ranked targets; lane c then walks the
// chunk for cutoff c in the row's order, so every sum has a fixed order and there is no reduction across lanes.  The
// means are a two-level sum in a fixed order (no floating-point atomics): two calls give the same bits.  Nothing here is
// contracted into a fused multiply-add: f1 rounds where the reference does.
#include <limits.h>

#include "common.h"

#pragma clang fp contract(off)

namespace daisy {
namespace {

constexpr int kPosWaves = kBlock / kWave;
constexpr int kPosLists = kPosWaves * kWave;        // requests per workgroup: a wave walks 64 consecutive ones
constexpr int kPosSlotsMax = 9;                     // the eight per-list KPIs of a hit mask and full_auc
constexpr int kPosAcc = (kPosSlotsMax * DAISY_METRICS_MAX_CUTOFFS + kWave - 1) / kWave;
constexpr uint32_t kPosListKpis = (1u << (DAISY_KPI_AUC + 1)) - 1u;             // precision .. auc
constexpr uint32_t kPosKnown = kPosListKpis | (1u << DAISY_KPI_FULL_AUC);

inline int pos_slots(uint32_t mask) { return __builtin_popcount(mask & kPosKnown); }
inline int64_t pos_blocks(int64_t n) { return (n + kPosLists - 1) / kPosLists; }

struct PosArgs {
    const int64_t *indptr;
    const int32_t *pos;
    const int64_t *gt_len;
    const int32_t *eligible;
    int64_t n;
    int nc;
    int cut[DAISY_METRICS_MAX_CUTOFFS];
    const double *disc;
    const double *disc_cum;
    int64_t disc_len;
    uint32_t mask;
    double *per_user;
    double *partial;
    int64_t n_blocks;
};

__device__ __forceinline__ void pos_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int pos_slot(uint32_t mask, int kpi) { return __popc(mask & kPosKnown & ((1u << kpi) - 1u)); }

__global__ __launch_bounds__(kBlock) void k_position_kpis(const PosArgs a) {
    __shared__ int32_t s_pos[kPosWaves][kWave];
    __shared__ int32_t s_rank[kPosWaves][kWave];
    __shared__ double s_part[kPosWaves][kPosAcc * kWave];
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const uint32_t mask = a.mask;
    const int nc = a.nc;
    const bool w_pre = (mask >> DAISY_KPI_PRECISION) & 1u, w_rec = (mask >> DAISY_KPI_RECALL) & 1u;
    const bool w_hit = (mask >> DAISY_KPI_HIT) & 1u, w_mrr = (mask >> DAISY_KPI_MRR) & 1u;
    const bool w_map = (mask >> DAISY_KPI_MAP) & 1u, w_ndcg = (mask >> DAISY_KPI_NDCG) & 1u;
    const bool w_f1 = (mask >> DAISY_KPI_F1) & 1u, w_auc = (mask >> DAISY_KPI_AUC) & 1u;
    const bool w_full = (mask >> DAISY_KPI_FULL_AUC) & 1u;

    int my_k = 0;                                       // lane c answers cutoff c (0: no cutoff, nothing is a hit)
#pragma unroll
    for (int c = 0; c < DAISY_METRICS_MAX_CUTOFFS; ++c)
        if (lane == c && c < nc) my_k = a.cut[c];
    double acc[kPosSlotsMax];
#pragma unroll
    for (int r = 0; r < kPosSlotsMax; ++r) acc[r] = 0.0;

    const int64_t first = blockIdx.x * (int64_t)kPosLists + (int64_t)wave * kWave;
#pragma unroll 1
    for (int t = 0; t < kWave; ++t) {
        const int64_t list = first + t;
        if (list >= a.n) break;                         // the same for every lane of the wave
        const int64_t beg = a.indptr[list], L = a.indptr[list + 1] - beg;
        const double len = (double)(a.gt_len ? a.gt_len[list] : L);
        const int64_t E = a.eligible[list];

        int64_t h = 0, an = 0, ranked = 0, spread = 0;  // an: sum over the hits of rank - pos; spread: of pos - rank, all ranked
        int fmin = INT_MAX;
        double smap = 0.0, sdcg = 0.0;
#pragma unroll 1
        for (int64_t base = 0; base < L; base += kWave) {
            const int64_t e = base + lane;
            const int32_t p = e < L ? a.pos[beg + e] : -1;
            int32_t r = 0;                              // the ranked targets of the row that come before this one
            if (p >= 0)
                for (int64_t j = 0; j < L; ++j) {
                    const int32_t q = a.pos[beg + j];
                    r += (q >= 0 && q < p) ? 1 : 0;
                }
            pos_wave_sync();                            // the readers of the previous chunk are done
            s_pos[wave][lane] = p;
            s_rank[wave][lane] = r;
            pos_wave_sync();
            const int m = (int)(L - base < kWave ? L - base : kWave);
            for (int j = 0; j < m; ++j) {
                const int32_t pj = s_pos[wave][j], rj = s_rank[wave][j];
                if (pj < 0) continue;
                ++ranked;
                spread += (int64_t)pj - rj;
                fmin = pj < fmin ? pj : fmin;
                if (pj < my_k) {
                    ++h;
                    an += (int64_t)rj - pj;
                    if (w_map) smap += (double)(rj + 1) / (double)(pj + 1);
                    if (w_ndcg && pj < a.disc_len) sdcg += a.disc[pj];
                }
            }
        }

        if (lane < nc) {
            const int64_t k = my_k;
            const int64_t keff = k < E ? k : E;         // K above the eligible items: the implied list is E long
            const double pre = (double)h / (double)keff, rec = (double)h / len;
            double *out = a.per_user ? a.per_user + (int64_t)lane * a.n + list : nullptr;
            const int64_t slot_stride = (int64_t)nc * a.n;
#define DAISY_POS_EMIT(KPI, SLOT, V)                                            \
    do {                                                                        \
        const double v_ = (V);                                                  \
        acc[SLOT] += v_;                                                        \
        if (out) out[pos_slot(mask, KPI) * slot_stride] = v_;                   \
    } while (0)
            if (w_pre) DAISY_POS_EMIT(DAISY_KPI_PRECISION, 0, pre);
            if (w_rec) DAISY_POS_EMIT(DAISY_KPI_RECALL, 1, rec);
            if (w_hit) DAISY_POS_EMIT(DAISY_KPI_HIT, 2, h ? 1.0 : 0.0);
            if (w_mrr) DAISY_POS_EMIT(DAISY_KPI_MRR, 3, fmin < k ? 1.0 / (double)(fmin + 1) : 0.0);
            if (w_map) DAISY_POS_EMIT(DAISY_KPI_MAP, 4, h ? smap / (double)h : 0.0);
            if (w_ndcg) {
                const double idcg = (h && h <= a.disc_len) ? a.disc_cum[h - 1] : 0.0;
                DAISY_POS_EMIT(DAISY_KPI_NDCG, 5, idcg != 0.0 ? sdcg / idcg : 0.0);
            }
            if (w_f1) DAISY_POS_EMIT(DAISY_KPI_F1, 6, 2.0 * pre * rec / (pre + rec));
            if (w_auc)                                  // per hit the misses behind it: (keff - 1 - pos) - (h - 1 - rank)
                DAISY_POS_EMIT(DAISY_KPI_AUC, 7, (double)(h * (keff - 1) + an - h * (h - 1)) / (double)(h * (keff - h)));
            if (w_full)
                DAISY_POS_EMIT(DAISY_KPI_FULL_AUC, 8,
                               (double)(ranked * (E - ranked) - spread) / (double)(ranked * (E - ranked)));
#undef DAISY_POS_EMIT
        }
    }

#pragma unroll
    for (int r = 0; r < kPosSlotsMax; ++r) {
        const int kpi = r < 8 ? r : DAISY_KPI_FULL_AUC;
        if (((mask >> kpi) & 1u) && lane < nc) s_part[wave][pos_slot(mask, kpi) * nc + lane] = acc[r];
    }
    __syncthreads();
    const int n_idx = __popc(mask & kPosKnown) * nc;
    for (int idx = tid; idx < n_idx; idx += kBlock) {
        double s = s_part[0][idx];
#pragma unroll
        for (int wv = 1; wv < kPosWaves; ++wv) s += s_part[wv][idx];
        a.partial[(int64_t)idx * a.n_blocks + blockIdx.x] = s;
    }
}

// means[idx] = (the workgroups' partial sums, thread t adding the partials t, t + 256, ... and the threads meeting in a
// fixed tree) / n
__global__ __launch_bounds__(kBlock) void k_position_means(const double *__restrict__ partial, int64_t n_blocks, int64_t n,
                                                           double *__restrict__ means) {
    __shared__ double s_t[kBlock];
    const int tid = threadIdx.x, idx = blockIdx.x;
    double s = 0.0;
    for (int64_t b = tid; b < n_blocks; b += kBlock) s += partial[(int64_t)idx * n_blocks + b];
    s_t[tid] = s;
    __syncthreads();
    for (int off = kBlock / 2; off > 0; off >>= 1) {
        if (tid < off) s_t[tid] += s_t[tid + off];
        __syncthreads();
    }
    if (tid == 0) means[idx] = s_t[0] / (double)n;
}

}  // namespace
}  // namespace daisy

using namespace daisy;

extern "C" {

size_t daisy_position_kpis_workspace_bytes(int64_t n, int32_t nc, uint32_t metrics) {
    if (n < 1 || n > INT_MAX || nc < 1 || nc > DAISY_METRICS_MAX_CUTOFFS || metrics == 0 || (metrics & ~kPosKnown)) return 0;
    return align_up((size_t)pos_slots(metrics) * (size_t)nc * (size_t)pos_blocks(n) * sizeof(double));
}

int daisy_position_kpis(const int64_t *out_indptr, const int32_t *positions, const int64_t *gt_len, const int32_t *eligible,
                        int64_t n, const int32_t *cutoffs_host, int32_t nc, const double *disc, const double *disc_cum,
                        int64_t disc_len, uint32_t metrics, double *per_user, double *means, void *workspace,
                        size_t workspace_bytes, daisy_stream_t stream) {
    DAISY_CHECK_ARG(out_indptr && positions && eligible && cutoffs_host && means && workspace, "position_kpis: NULL argument");
    DAISY_CHECK_ARG(n >= 1 && n <= INT_MAX, "position_kpis: n=%lld", (long long)n);
    DAISY_CHECK_ARG(nc >= 1 && nc <= DAISY_METRICS_MAX_CUTOFFS, "position_kpis: %d cutoffs outside [1, %d]", nc,
                    DAISY_METRICS_MAX_CUTOFFS);
    for (int c = 0; c < nc; ++c)
        DAISY_CHECK_ARG(cutoffs_host[c] >= 1 && (c == 0 || cutoffs_host[c] > cutoffs_host[c - 1]),
                        "position_kpis: the cutoffs must be >= 1 and strictly ascending (cutoff %d is %d)", c, cutoffs_host[c]);
    DAISY_CHECK_ARG(metrics != 0 && !(metrics & ~kPosKnown),
                    "position_kpis: metrics mask 0x%x (popularity, diversity and coverage need the lists)", metrics);
    DAISY_CHECK_ARG(!((metrics >> DAISY_KPI_NDCG) & 1u) || (disc && disc_cum && disc_len >= 1),
                    "position_kpis: ndcg needs the discount tables (NULL disc or disc_cum)");
    const size_t need = daisy_position_kpis_workspace_bytes(n, nc, metrics);
    DAISY_CHECK_ARG(workspace_bytes >= need, "position_kpis: workspace of %zu bytes, %zu needed", workspace_bytes, need);

    hipStream_t s = as_stream(stream);
    PosArgs a;
    a.indptr = out_indptr;
    a.pos = positions;
    a.gt_len = gt_len;
    a.eligible = eligible;
    a.n = n;
    a.nc = nc;
    for (int c = 0; c < DAISY_METRICS_MAX_CUTOFFS; ++c) a.cut[c] = c < nc ? cutoffs_host[c] : 0;
    a.disc = disc;
    a.disc_cum = disc_cum;
    a.disc_len = disc ? disc_len : 0;
    a.mask = metrics;
    a.per_user = per_user;
    a.partial = static_cast<double *>(workspace);
    a.n_blocks = pos_blocks(n);
    hipLaunchKernelGGL(k_position_kpis, dim3((unsigned)a.n_blocks), dim3(kBlock), 0, s, a);
    DAISY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_position_means, dim3((unsigned)(pos_slots(metrics) * nc)), dim3(kBlock), 0, s, a.partial, a.n_blocks, n,
                       means);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // extern "C"
