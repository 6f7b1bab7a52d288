// The ranking KPIs of daisy/utils/metrics.py on the device: one wave per ranked list, the hit mask of 64
// positions from one ballot, every KPI at every cutoff from prefix popcounts and prefix sums of that mask, and the means
// over the lists as a two-level sum in a fixed order.  No floating-point atomics: the only atomics are the integer OR on
// the coverage bitmaps and the integer add on their counts, whose results do not depend on their order, so every output
// is the same run after run.  Nothing here is contracted into a fused multiply-add: f1 rounds where the reference does.
#include <limits.h>

#include "common.h"

#pragma clang fp contract(off)

namespace daisy {
namespace {

constexpr int kMetWaves = kBlock / kWave;
constexpr int kMetLists = kMetWaves * kWave;        // lists per workgroup: a wave walks 64 consecutive ones
constexpr int kMetAcc = (DAISY_KPI_PER_USER * DAISY_METRICS_MAX_CUTOFFS + kWave - 1) / kWave;
constexpr uint32_t kMetKnown = (1u << DAISY_KPI_COUNT) - 1u;
constexpr uint32_t kMetPerUser = (1u << DAISY_KPI_PER_USER) - 1u;
static_assert(DAISY_METRICS_MAX_CAT_WORDS == 4 && DAISY_METRICS_MAX_CATS == 64 * DAISY_METRICS_MAX_CAT_WORDS,
              "k_metrics_lists is instantiated for masks of 1 .. 4 words");

inline bool met_has(uint32_t mask, int kpi) { return (mask >> kpi) & 1u; }
inline int met_slots(uint32_t mask) { return __builtin_popcount(mask & kMetPerUser); }
inline int64_t met_blocks(int64_t n) { return (n + kMetLists - 1) / kMetLists; }
inline int64_t met_words(int64_t item_num) { return (item_num + 63) / 64; }

struct MetArgs {
    const void *pred;
    int pred_i64;
    int64_t n;
    int K;
    const int64_t *indptr;
    const int32_t *gt;
    int64_t user_num;
    const int64_t *users;
    int nc;
    int cut[DAISY_METRICS_MAX_CUTOFFS];
    const double *disc;
    const double *item_pop;
    int64_t item_num;
    const unsigned long long *cat;
    int C;
    const double *sqrt_tab;
    uint32_t mask;
    double *per_user;
    double *partial;
    int64_t n_blocks;
    unsigned long long *bitmap;
    int64_t words;
};

// The LDS traffic of one wave runs in program order; this keeps the compiler from moving an access across the point
// where the lanes of a wave exchange data through it.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Inclusive prefix sums over the lanes of a wave without the LDS crossbar: four doubling steps inside every 16-lane row
// (row_shr 1, 2, 4, 8: a lane whose source lies outside its row adds 0), then lane 15 of rows 0 and 2 into rows 1 and 3
// (row_bcast15), then lane 31 into rows 2 and 3 (row_bcast31).  Lane l ends with x[0] + ... + x[l] in a fixed tree.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int scan_dpp_i32(int x) {
    return __builtin_amdgcn_update_dpp(0, x, CTRL, ROW_MASK, 0xF, true);        // lanes outside ROW_MASK get 0 as well
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double scan_dpp_f64(double x) {
    const long long b = __builtin_bit_cast(long long, x);
    const int lo = scan_dpp_i32<CTRL, ROW_MASK>((int)(b & 0xFFFFFFFFll)), hi = scan_dpp_i32<CTRL, ROW_MASK>((int)(b >> 32));
    return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned int)lo);
}
constexpr int kDppRowShr = 0x110, kDppRowBcast15 = 0x142, kDppRowBcast31 = 0x143;
__device__ __forceinline__ double wave_scan_f64(double x) {
    x += scan_dpp_f64<kDppRowShr + 1, 0xF>(x);
    x += scan_dpp_f64<kDppRowShr + 2, 0xF>(x);
    x += scan_dpp_f64<kDppRowShr + 4, 0xF>(x);
    x += scan_dpp_f64<kDppRowShr + 8, 0xF>(x);
    x += scan_dpp_f64<kDppRowBcast15, 0xA>(x);
    x += scan_dpp_f64<kDppRowBcast31, 0xC>(x);
    return x;
}
__device__ __forceinline__ int wave_scan_i32(int x) {
    x += scan_dpp_i32<kDppRowShr + 1, 0xF>(x);
    x += scan_dpp_i32<kDppRowShr + 2, 0xF>(x);
    x += scan_dpp_i32<kDppRowShr + 4, 0xF>(x);
    x += scan_dpp_i32<kDppRowShr + 8, 0xF>(x);
    x += scan_dpp_i32<kDppRowBcast15, 0xA>(x);
    x += scan_dpp_i32<kDppRowBcast31, 0xC>(x);
    return x;
}

__device__ __forceinline__ bool met_in_row(const int32_t *__restrict__ gt, int64_t beg, int64_t end, int32_t id) {
    while (beg < end) {                                 // items ascend within a row
        const int64_t mid = beg + (end - beg) / 2;
        const int32_t c = gt[mid];
        if (c == id) return true;
        if (c < id) beg = mid + 1; else end = mid;
    }
    return false;
}

// a row of at most 64 truths held one per lane (padded with INT_MAX): every lane meets every truth through readlane,
// three instructions per truth and no memory access
__device__ __forceinline__ bool met_in_lanes(int32_t gt_mine, int len, int32_t id) {
    bool hit = false;
    for (int j = 0; j < len; ++j) hit |= id == __builtin_amdgcn_readlane(gt_mine, j);
    return hit;
}

// lane `src` of a 64-bit value; src is the same in every lane
__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long x, int src) {
    const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(x & 0xFFFFFFFFull), src);
    const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(x >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ int met_slot(uint32_t mask, int kpi) { return __popc(mask & ((1u << kpi) - 1u)); }

// One wave per list, 64 consecutive lists per wave.  A list longer than 64 runs in chunks of 64 positions in ascending
// order; what a later chunk needs of the earlier ones (hits, the first hit, the running sums) is carried in registers, the
// ids of the list and its distinct hits so far in LDS.  A cutoff k is answered inside the chunk that holds position k - 1:
// lane k - 1 - base of every prefix scan holds the sum over the first k positions.  Lane c answers cutoff c - the KPIs of
// all cutoffs are formed side by side, not one cutoff after the other on 64 idle copies - and keeps the running sums of
// "its" cutoff over the wave's lists.
// Global loads sit off the critical path: the owners and row bounds of a wave's 64 lists are fetched once, one per lane;
// the first 64 positions and the truth row (when it has at most 64 items: it then stays in registers, one per lane) of list
// t + 1 are requested before list t is worked on; the discounts and the square roots are read from LDS.
// NW: the words of a category mask when diversity is asked for (an instance per width: the pair loop is its hot spot),
// 0 when it is not
template <int NW>
__global__ __launch_bounds__(kBlock) void k_metrics_lists(const MetArgs a) {
    __shared__ double s_cum[DAISY_METRICS_MAX_K];                       // disc[0] + ... + disc[p]
    __shared__ double s_disc[DAISY_METRICS_MAX_K];
    __shared__ double s_sqrt[DAISY_METRICS_MAX_CATS + 1];
    __shared__ int32_t s_ids[kMetWaves][DAISY_METRICS_MAX_K];
    __shared__ int32_t s_hit[kMetWaves][DAISY_METRICS_MAX_K];
    __shared__ double s_part[kMetWaves][kMetAcc * kWave];
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t mask = a.mask;
    const int K = a.K, nc = a.nc;
    const bool w_pre = (mask >> DAISY_KPI_PRECISION) & 1u, w_rec = (mask >> DAISY_KPI_RECALL) & 1u;
    const bool w_hit = (mask >> DAISY_KPI_HIT) & 1u, w_mrr = (mask >> DAISY_KPI_MRR) & 1u;
    const bool w_map = (mask >> DAISY_KPI_MAP) & 1u, w_ndcg = (mask >> DAISY_KPI_NDCG) & 1u;
    const bool w_f1 = (mask >> DAISY_KPI_F1) & 1u, w_auc = (mask >> DAISY_KPI_AUC) & 1u;
    const bool w_pop = (mask >> DAISY_KPI_POPULARITY) & 1u;
    constexpr bool w_div = NW > 0;                // diversity has an instance of its own: its masks would cost every call registers
    const bool w_cov = (mask >> DAISY_KPI_COVERAGE) & 1u;

    if (w_ndcg && wave == 0) {
        double carry = 0.0;
        for (int base = 0; base < K; base += kWave) {
            const int p = base + lane;
            const double s = wave_scan_f64(p < K ? a.disc[p] : 0.0);
            if (p < K) s_cum[p] = carry + s;
            carry += __shfl(s, kWave - 1, kWave);
        }
    }
    if (w_ndcg)
        for (int p = tid; p < K; p += kBlock) s_disc[p] = a.disc[p];
    if (w_div)
        for (int i = tid; i <= a.C; i += kBlock) s_sqrt[i] = a.sqrt_tab[i];
    __syncthreads();

    // lane c answers cutoff c: its cutoff and its running sum of every KPI over the wave's lists
    int my_k = INT_MAX;
#pragma unroll
    for (int c = 0; c < DAISY_METRICS_MAX_CUTOFFS; ++c)
        if (lane == c && c < nc) my_k = a.cut[c];
    double acc[DAISY_KPI_PER_USER];
#pragma unroll
    for (int r = 0; r < DAISY_KPI_PER_USER; ++r) acc[r] = 0.0;

    const int64_t first = blockIdx.x * (int64_t)kMetLists + (int64_t)wave * kWave;
    long long my_beg = 0, my_end = 0;                                   // the truth row of the list first + lane
    if (first + lane < a.n) {
        const int64_t u = a.users[first + lane];
        if (u >= 0 && u < a.user_num) { my_beg = a.indptr[u]; my_end = a.indptr[u + 1]; }
    }
    // an id as it lies in memory (the low word alone for int32 lists): widening it only where it is used keeps the
    // request of the next list's ids from being waited for at once
    auto load_raw = [&](int64_t list, int pos) -> int64_t {
        if (pos >= K) return -1;
        const int64_t e = list * (int64_t)K + pos;
        if (a.pred_i64) return static_cast<const int64_t *>(a.pred)[e];
        int64_t raw = 0;
        __builtin_memcpy(&raw, static_cast<const int32_t *>(a.pred) + e, sizeof(int32_t));
        return raw;
    };
    auto widen = [&](int64_t raw, int pos) -> int64_t {
        return (a.pred_i64 || pos >= K) ? raw : (int64_t)(int32_t)(raw & 0xFFFFFFFFll);
    };
    auto load_gt = [&](int64_t beg, int64_t end) -> int32_t {          // lane l: item l of a row of at most 64, else a pad
        return (end - beg <= kWave && lane < end - beg) ? a.gt[beg + lane] : INT_MAX;
    };
    int64_t id_next = -1, beg_next = 0, end_next = 0;
    int32_t gt_next = INT_MAX;
    if (first < a.n) {
        id_next = load_raw(first, lane);
        beg_next = (int64_t)readlane_u64((unsigned long long)my_beg, 0);
        end_next = (int64_t)readlane_u64((unsigned long long)my_end, 0);
        gt_next = load_gt(beg_next, end_next);
    }
#pragma unroll 1
    for (int t = 0; t < kWave; ++t) {
        const int64_t list = first + t;
        if (list >= a.n) break;                                         // the same for every lane of the wave
        const int64_t id_first = id_next, beg = beg_next, end = end_next;
        const int32_t gt_mine = gt_next;
        if (t + 1 < kWave && list + 1 < a.n) {                          // the next list's loads fly while this one is worked on
            id_next = load_raw(list + 1, lane);
            beg_next = (int64_t)readlane_u64((unsigned long long)my_beg, t + 1);
            end_next = (int64_t)readlane_u64((unsigned long long)my_end, t + 1);
            gt_next = load_gt(beg_next, end_next);
        }
        const bool short_row = end - beg <= kWave;
        const int len_i = (int)(short_row ? end - beg : 0);
        const double len = (double)(end - beg);

        int H0 = 0, F0 = -1, A0 = 0, n_hit = 0;
        double Smap = 0.0, Sdcg = 0.0, Spop = 0.0, Sdiv = 0.0;
#pragma unroll 1
        for (int base = 0; base < K; base += kWave) {
            const int pos = base + lane;
            const bool in = pos < K;
            const int64_t id = widen(base == 0 ? id_first : load_raw(list, pos), pos);
            const bool ok = in && id >= 0 && id < a.item_num;
            const int32_t id32 = ok ? (int32_t)id : -1;
            wave_lds_sync();                                            // the readers of the previous chunk and list are done
            if (in) s_ids[wave][pos] = id32;
            const bool hit = ok && (short_row ? met_in_lanes(gt_mine, len_i, id32) : met_in_row(a.gt, beg, end, id32));
            const unsigned long long hm = __ballot(hit);
            const int hits_to = H0 + __popcll(hm & below) + (hit ? 1 : 0);      // hits among the positions <= pos

            if (w_cov && ok) {
                int c0 = -1;                                            // the first cutoff that holds this position
                for (int c = nc - 1; c >= 0; --c)
                    if (a.cut[c] > pos) c0 = c;
                if (c0 >= 0) {
                    unsigned long long *word = a.bitmap + (int64_t)c0 * a.words + (id32 >> 6);
                    const unsigned long long bit = 1ull << (id32 & 63);
                    if (!(*word & bit)) atomicOr(word, bit);            // most bits are set already: no atomic then
                }
            }

            double mscan = 0.0, gscan = 0.0, pscan = 0.0, dscan = 0.0;
            int ascan = 0;
            if (w_map) mscan = wave_scan_f64(hit ? (double)hits_to / (double)(pos + 1) : 0.0);
            if (w_ndcg) gscan = wave_scan_f64(hit ? s_disc[pos] : 0.0);
            if (w_auc) ascan = wave_scan_i32((in && !hit) ? hits_to : 0);    // the hits before a position without one
            if (w_pop) {
                // a hit item counts once (np.intersect1d): not when an earlier position of the list holds the same id
                bool firstocc = hit;
                for (int q = 0; q < n_hit; ++q)
                    if (s_hit[wave][q] == id32) firstocc = false;
                unsigned long long rem = hm;
                while (rem) {
                    const int b = __ffsll((long long)rem) - 1;
                    rem &= rem - 1ull;
                    const int32_t idb = __shfl(id32, b, kWave);
                    if (lane > b && id32 == idb) firstocc = false;
                }
                if (base + kWave < K) {                                 // a later chunk will ask
                    const unsigned long long fm = __ballot(firstocc);
                    if (firstocc) s_hit[wave][n_hit + __popcll(fm & below)] = id32;
                    n_hit += __popcll(fm);
                }
                pscan = wave_scan_f64(firstocc ? a.item_pop[id32] : 0.0);
            }
            if constexpr (NW > 0) {
                // the pairs (i, j), i < j, j in this chunk: lane j adds its column in ascending i.  The masks of 64
                // positions sit one per lane (this chunk's own, or an earlier chunk's fetched again) and reach the
                // other lanes through readlane: no memory access inside the pair loop but the table of roots in LDS.
                unsigned long long cj[NW];
#pragma unroll
                for (int w = 0; w < NW; ++w)
                    cj[w] = ok ? a.cat[(int64_t)id32 * NW + w] : 0ull;
                const int last = (base + kWave < K ? base + kWave : K) - 1;     // the last position of this chunk
                double col = 0.0;
#pragma unroll 1
                for (int qb = 0; qb <= base; qb += kWave) {
                    unsigned long long ci[NW];
                    const int32_t idq = qb == base ? id32 : s_ids[wave][qb + lane];
#pragma unroll
                    for (int w = 0; w < NW; ++w)
                        ci[w] = qb == base ? cj[w] : (idq >= 0 ? a.cat[(int64_t)idq * NW + w] : 0ull);
                    const int cnt = qb == base ? last - base : kWave;   // i = qb .. qb + cnt - 1, all below `last`
#pragma unroll 1
                    for (int i0 = 0; i0 < cnt; i0 += 8) {               // eight at a time: their roots come from LDS together
#pragma unroll
                        for (int i = i0; i < i0 + 8; ++i) {             // (i >= cnt: qb + i >= last >= pos, nothing is added)
                            int d = 0;
#pragma unroll
                            for (int w = 0; w < NW; ++w)
                                d += __popcll(readlane_u64(ci[w], i) ^ cj[w]);
                            if (d > a.C) d = a.C;
                            if (in && qb + i < pos) col += s_sqrt[d];
                        }
                    }
                }
                dscan = wave_scan_f64(col);
            }

            // every cutoff inside this chunk at once, lane c for cutoff c; the prefix sums are fetched with all lanes on
            const bool mine = my_k > base && my_k <= base + kWave;
            const int kk = mine ? my_k - base : 1, src = kk - 1;
            const double mval = w_map ? __shfl(mscan, src, kWave) : 0.0, gval = w_ndcg ? __shfl(gscan, src, kWave) : 0.0;
            const double pval = w_pop ? __shfl(pscan, src, kWave) : 0.0, dval = w_div ? __shfl(dscan, src, kWave) : 0.0;
            const int aval = w_auc ? __shfl(ascan, src, kWave) : 0;
            if (mine) {
                const int k = my_k;
                const unsigned long long m = kk == kWave ? hm : (hm & ((1ull << kk) - 1ull));
                const int h = H0 + __popcll(m);
                const double pre = (double)h / (double)k, rec = (double)h / len;
                double *out = a.per_user ? a.per_user + (int64_t)lane * a.n + list : nullptr;
                const int64_t slot_stride = (int64_t)nc * a.n;
#define DAISY_KPI_EMIT(KPI, V)                                                  \
    do {                                                                        \
        const double v_ = (V);                                                  \
        acc[KPI] += v_;                                                         \
        if (out) out[met_slot(mask, KPI) * slot_stride] = v_;                   \
    } while (0)
                if (w_pre) DAISY_KPI_EMIT(DAISY_KPI_PRECISION, pre);
                if (w_rec) DAISY_KPI_EMIT(DAISY_KPI_RECALL, rec);
                if (w_hit) DAISY_KPI_EMIT(DAISY_KPI_HIT, h ? 1.0 : 0.0);
                if (w_mrr) {
                    const int f = F0 >= 0 ? F0 : (m ? base + __ffsll((long long)m) - 1 : -1);
                    DAISY_KPI_EMIT(DAISY_KPI_MRR, f >= 0 ? 1.0 / (double)(f + 1) : 0.0);
                }
                if (w_map) DAISY_KPI_EMIT(DAISY_KPI_MAP, h ? (Smap + mval) / (double)h : 0.0);
                if (w_ndcg) {
                    const double idcg = h ? s_cum[h - 1] : 0.0;
                    DAISY_KPI_EMIT(DAISY_KPI_NDCG, idcg != 0.0 ? (Sdcg + gval) / idcg : 0.0);
                }
                if (w_f1) DAISY_KPI_EMIT(DAISY_KPI_F1, 2.0 * pre * rec / (pre + rec));
                if (w_auc) DAISY_KPI_EMIT(DAISY_KPI_AUC, (double)(A0 + aval) / (double)((int64_t)h * (int64_t)(k - h)));
                if (w_pop) DAISY_KPI_EMIT(DAISY_KPI_POPULARITY, h ? (Spop + pval) / len : 0.0);
                if (w_div) DAISY_KPI_EMIT(DAISY_KPI_DIVERSITY, (Sdiv + dval) / (double)((int64_t)k * (k - 1) / 2));
#undef DAISY_KPI_EMIT
            }

            if (F0 < 0 && hm) F0 = base + __ffsll((long long)hm) - 1;
            H0 += __popcll(hm);
            if (w_map) Smap += __shfl(mscan, kWave - 1, kWave);
            if (w_ndcg) Sdcg += __shfl(gscan, kWave - 1, kWave);
            if (w_auc) A0 += __shfl(ascan, kWave - 1, kWave);
            if (w_pop) Spop += __shfl(pscan, kWave - 1, kWave);
            if (w_div) Sdiv += __shfl(dscan, kWave - 1, kWave);
        }
    }

#pragma unroll
    for (int r = 0; r < DAISY_KPI_PER_USER; ++r)
        if (((mask >> r) & 1u) && lane < nc) s_part[wave][met_slot(mask, r) * nc + lane] = acc[r];
    __syncthreads();
    const int n_idx = met_slot(mask, DAISY_KPI_PER_USER) * nc;
    for (int idx = tid; idx < n_idx; idx += kBlock) {
        double s = s_part[0][idx];
#pragma unroll
        for (int wv = 1; wv < kMetWaves; ++wv) s += s_part[wv][idx];
        a.partial[(int64_t)idx * a.n_blocks + blockIdx.x] = s;
    }
}

// means[idx] = (the workgroups' partial sums, thread t adding the partials t, t + 256, ... and the threads meeting in a
// fixed tree) / n
__global__ __launch_bounds__(kBlock) void k_metrics_means(const double *__restrict__ partial, int64_t n_blocks, int64_t n,
                                                          double *__restrict__ means) {
    __shared__ double s_w[kMetWaves];
    const int tid = threadIdx.x, idx = blockIdx.x;
    double s = 0.0;
    for (int64_t b = tid; b < n_blocks; b += kBlock) s += partial[(int64_t)idx * n_blocks + b];
    s = wave_sum_f64(s);
    if (tid % kWave == 0) s_w[tid / kWave] = s;
    __syncthreads();
    if (tid == 0) {
        double tot = s_w[0];
#pragma unroll
        for (int wv = 1; wv < kMetWaves; ++wv) tot += s_w[wv];
        means[idx] = tot / (double)n;
    }
}

// counts[c] = the bits set in bitmap[0] | ... | bitmap[c]: a position marks the bitmap of the FIRST cutoff that holds it
__global__ __launch_bounds__(kBlock) void k_metrics_cover(const unsigned long long *__restrict__ bitmap, int64_t words, int nc,
                                                          unsigned long long *__restrict__ counts) {
    int cnt[DAISY_METRICS_MAX_CUTOFFS];
#pragma unroll
    for (int c = 0; c < DAISY_METRICS_MAX_CUTOFFS; ++c) cnt[c] = 0;
    for (int64_t w = blockIdx.x * (int64_t)kBlock + threadIdx.x; w < words; w += (int64_t)gridDim.x * kBlock) {
        unsigned long long seen = 0ull;
#pragma unroll
        for (int c = 0; c < DAISY_METRICS_MAX_CUTOFFS; ++c) {
            if (c < nc) {
                seen |= bitmap[(int64_t)c * words + w];
                cnt[c] += __popcll(seen);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < DAISY_METRICS_MAX_CUTOFFS; ++c) {
        int v = cnt[c];
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
        if (c < nc && v && threadIdx.x % kWave == 0) atomicAdd(&counts[c], (unsigned long long)v);
    }
}

struct MetLayout {
    size_t partial, bitmap, total;
};
inline MetLayout met_layout(int64_t n, int nc, int64_t item_num, uint32_t metrics) {
    MetLayout l;
    l.partial = 0;
    l.bitmap = align_up((size_t)met_slots(metrics) * (size_t)nc * (size_t)met_blocks(n) * sizeof(double));
    l.total = l.bitmap + (met_has(metrics, DAISY_KPI_COVERAGE)
                              ? align_up((size_t)nc * (size_t)met_words(item_num) * sizeof(unsigned long long)) : 0);
    return l;
}

}  // namespace
}  // namespace daisy

using namespace daisy;

extern "C" {

size_t daisy_ranking_kpis_workspace_bytes(int64_t n, int32_t nc, int64_t item_num, uint32_t metrics) {
    if (n < 1 || n > INT_MAX || nc < 1 || nc > DAISY_METRICS_MAX_CUTOFFS || item_num < 1 || item_num > INT_MAX ||
        (metrics & ~kMetKnown))
        return 0;
    return met_layout(n, nc, item_num, metrics).total;
}

int daisy_ranking_kpis(const void *pred, int32_t pred_is_i64, int64_t n, int32_t K, const int64_t *indptr,
                       const int32_t *gt_items, int64_t user_num, const int64_t *users, const int32_t *cutoffs_host,
                       int32_t nc, const double *disc, const double *item_pop, int64_t item_num, const uint64_t *cat_bits,
                       int32_t cat_words, int32_t n_cats, const double *sqrt_tab, uint32_t metrics, double *per_user,
                       double *means, int64_t *cover_counts, void *workspace, size_t workspace_bytes,
                       daisy_stream_t stream) {
    DAISY_CHECK_ARG(pred && indptr && gt_items && users && cutoffs_host && workspace, "ranking_kpis: NULL argument");
    DAISY_CHECK_ARG(n >= 1 && n <= INT_MAX && user_num >= 1 && item_num >= 1 && item_num <= INT_MAX,
                    "ranking_kpis: n=%lld user_num=%lld item_num=%lld", (long long)n, (long long)user_num,
                    (long long)item_num);
    DAISY_CHECK_ARG(K >= 1 && K <= DAISY_METRICS_MAX_K, "ranking_kpis: K=%d outside [1, %d]", K, DAISY_METRICS_MAX_K);
    DAISY_CHECK_ARG(nc >= 1 && nc <= DAISY_METRICS_MAX_CUTOFFS, "ranking_kpis: %d cutoffs outside [1, %d]", nc,
                    DAISY_METRICS_MAX_CUTOFFS);
    for (int c = 0; c < nc; ++c) {
        DAISY_CHECK_ARG(cutoffs_host[c] >= 1 && (c == 0 || cutoffs_host[c] > cutoffs_host[c - 1]),
                        "ranking_kpis: the cutoffs must be >= 1 and strictly ascending (cutoff %d is %d)", c, cutoffs_host[c]);
        DAISY_CHECK_ARG(cutoffs_host[c] <= K, "ranking_kpis: cutoff %d exceeds K=%d", cutoffs_host[c], K);
    }
    DAISY_CHECK_ARG(metrics != 0 && !(metrics & ~kMetKnown), "ranking_kpis: metrics mask 0x%x", metrics);
    const int slots = met_slots(metrics);
    DAISY_CHECK_ARG(slots == 0 || means, "ranking_kpis: NULL argument (means)");
    DAISY_CHECK_ARG(!met_has(metrics, DAISY_KPI_NDCG) || disc, "ranking_kpis: ndcg needs the discount table (NULL disc)");
    DAISY_CHECK_ARG(!met_has(metrics, DAISY_KPI_POPULARITY) || item_pop,
                    "ranking_kpis: popularity needs its table (NULL item_pop)");
    DAISY_CHECK_ARG(!met_has(metrics, DAISY_KPI_DIVERSITY) || (cat_bits && sqrt_tab),
                    "ranking_kpis: diversity needs its tables (NULL cat_bits or sqrt_tab)");
    DAISY_CHECK_ARG(!met_has(metrics, DAISY_KPI_DIVERSITY) ||
                        (n_cats >= 1 && n_cats <= DAISY_METRICS_MAX_CATS && cat_words == (n_cats + 63) / 64),
                    "ranking_kpis: n_cats=%d outside [1, %d] or cat_words=%d is not ceil(n_cats / 64)", n_cats,
                    DAISY_METRICS_MAX_CATS, cat_words);
    DAISY_CHECK_ARG(!met_has(metrics, DAISY_KPI_COVERAGE) || cover_counts, "ranking_kpis: coverage needs cover_counts (NULL)");
    const MetLayout lay = met_layout(n, nc, item_num, metrics);
    DAISY_CHECK_ARG(workspace_bytes >= lay.total, "ranking_kpis: workspace of %zu bytes, %zu needed", workspace_bytes,
                    lay.total);

    hipStream_t s = as_stream(stream);
    MetArgs a;
    a.pred = pred;
    a.pred_i64 = pred_is_i64 != 0;
    a.n = n;
    a.K = K;
    a.indptr = indptr;
    a.gt = gt_items;
    a.user_num = user_num;
    a.users = users;
    a.nc = nc;
    for (int c = 0; c < DAISY_METRICS_MAX_CUTOFFS; ++c) a.cut[c] = c < nc ? cutoffs_host[c] : INT_MAX;
    a.disc = disc;
    a.item_pop = item_pop;
    a.item_num = item_num;
    a.cat = reinterpret_cast<const unsigned long long *>(cat_bits);
    a.C = n_cats;
    a.sqrt_tab = sqrt_tab;
    a.mask = metrics;
    a.per_user = per_user;
    a.partial = reinterpret_cast<double *>(static_cast<char *>(workspace) + lay.partial);
    a.n_blocks = met_blocks(n);
    a.bitmap = reinterpret_cast<unsigned long long *>(static_cast<char *>(workspace) + lay.bitmap);
    a.words = met_words(item_num);
    const bool cover = met_has(metrics, DAISY_KPI_COVERAGE);
    if (cover) {
        DAISY_HIP(hipMemsetAsync(a.bitmap, 0, (size_t)nc * (size_t)a.words * sizeof(unsigned long long), s));
        DAISY_HIP(hipMemsetAsync(cover_counts, 0, (size_t)nc * sizeof(int64_t), s));
    }
    const dim3 grid((unsigned)a.n_blocks), block(kBlock);
    switch (met_has(metrics, DAISY_KPI_DIVERSITY) ? cat_words : 0) {
    case 0: hipLaunchKernelGGL(k_metrics_lists<0>, grid, block, 0, s, a); break;
    case 1: hipLaunchKernelGGL(k_metrics_lists<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(k_metrics_lists<2>, grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL(k_metrics_lists<3>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(k_metrics_lists<4>, grid, block, 0, s, a); break;
    }
    DAISY_LAUNCH_CHECK();
    if (slots) {
        hipLaunchKernelGGL(k_metrics_means, dim3((unsigned)(slots * nc)), dim3(kBlock), 0, s, a.partial, a.n_blocks, n, means);
        DAISY_LAUNCH_CHECK();
    }
    if (cover) {
        hipLaunchKernelGGL(k_metrics_cover, dim3(grid_for(a.words, kBlock)), dim3(kBlock), 0, s, a.bitmap, a.words, (int)nc,
                           reinterpret_cast<unsigned long long *>(cover_counts));
        DAISY_LAUNCH_CHECK();
    }
    return DAISY_OK;
}

}  // extern "C"
