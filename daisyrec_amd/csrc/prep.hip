// Preprocessor.process (daisy/utils/loader.py:176-189) on the device: dense codes of the raw ids, dedup of
// (user, item) keeping the last row, the rating threshold, the N-filter / N-core, the final category codes, the stable
// sort by timestamp and item_pop.  Everything is integer work: the sorts and scans are sort.hip's rocPRIM wrappers, the
// marking, counting, peeling and expansion kernels are below.  Counts come from the runs of the first encoding's sorted
// order (a scan of the live flags, one difference per run): no atomic.  The only atomics are the integer decrements of
// the peel, whose sums do not depend on their order, and the k-core is unique, so two calls give identical bytes.
#include <limits.h>

#include "common.h"

namespace daisy {
namespace {

constexpr uint64_t kSignBit = 1ull << 63;        // int64 -> uint64 that sorts in the same order

// keep[] states
constexpr uint8_t kDead = 0, kAlive = 1, kDying = 2;

// Every lane of the wave calls this together.  tab[id] += delta for the active lanes: the lanes that hold the id of
// the first pending lane add once, with their count (a popular item or a user-sorted frame puts one id on most lanes of
// a wave); after two such rounds whoever is left adds alone.
__device__ __forceinline__ void wave_count_add(int32_t *__restrict__ tab, int32_t id, bool active, int32_t delta) {
    const int lane = threadIdx.x % kWave;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned long long pend = __ballot(active);
        if (!pend) return;
        const int lead = __ffsll((long long)pend) - 1;
        const int32_t v = __shfl(id, lead, kWave);
        const bool same = active && id == v;
        const unsigned long long m = __ballot(same);
        if (lane == lead) atomicAdd(tab + v, delta * (int32_t)__popcll(m));
        active = active && !same;
    }
    if (active) atomicAdd(tab + id, delta);
}

// the rows of a grid-stride loop whose trip count is the same for every lane of a workgroup
#define DAISY_PREP_LOOP(e, n)                                                                                     \
    for (int64_t base_ = blockIdx.x * (int64_t)kBlock; base_ < (n); base_ += (int64_t)gridDim.x * kBlock)        \
        if (const int64_t e = base_ + threadIdx.x; true)

__global__ __launch_bounds__(kBlock) void k_prep_id_keys(const int64_t *__restrict__ ids, int64_t n,
                                                         uint64_t *__restrict__ key, int32_t *__restrict__ val) {
    DAISY_PREP_LOOP(e, n) {
        if (e < n) {
            key[e] = (uint64_t)ids[e] ^ kSignBit;
            val[e] = (int32_t)e;
        }
    }
}

// flag[e] = 1 where a new run starts in the sorted keys, except at e = 0: the inclusive sum is the run's rank
__global__ __launch_bounds__(kBlock) void k_prep_run_heads(const uint64_t *__restrict__ skey, int64_t n,
                                                           uint32_t *__restrict__ flag) {
    DAISY_PREP_LOOP(e, n) {
        if (e < n) flag[e] = (e > 0 && skey[e] != skey[e - 1]) ? 1u : 0u;
    }
}

__global__ __launch_bounds__(kBlock) void k_prep_scatter_codes(const uint64_t *__restrict__ skey, const int32_t *__restrict__ sval,
                                                               const uint32_t *__restrict__ flag, const uint32_t *__restrict__ excl,
                                                               int64_t n, int32_t *__restrict__ codes, int64_t *__restrict__ tokens,
                                                               uint32_t *__restrict__ start, int64_t *__restrict__ n_distinct) {
    DAISY_PREP_LOOP(e, n) {
        if (e < n) {
            const uint32_t r = excl[e] + flag[e];
            codes[sval[e]] = (int32_t)r;
            if (e == 0 || flag[e]) {
                tokens[r] = (int64_t)(skey[e] ^ kSignBit);
                if (start) start[r] = (uint32_t)e;          // run r of the sorted order is [start[r], start[r + 1])
            }
            if (e == n - 1) {
                *n_distinct = (int64_t)r + 1;
                if (start) start[r + 1] = (uint32_t)n;
            }
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_prep_pair_keys(const int32_t *__restrict__ u, const int32_t *__restrict__ i, int64_t n,
                                                           uint64_t *__restrict__ key, int32_t *__restrict__ val) {
    DAISY_PREP_LOOP(e, n) {
        if (e < n) {
            key[e] = ((uint64_t)(uint32_t)u[e] << 32) | (uint64_t)(uint32_t)i[e];
            val[e] = (int32_t)e;
        }
    }
}

// the sort is stable and the rows went in ascending: the tail of a run of equal pairs is its largest row number
__global__ __launch_bounds__(kBlock) void k_prep_mark_last(const uint64_t *__restrict__ skey, const int32_t *__restrict__ sval,
                                                           int64_t n, uint8_t *__restrict__ keep) {
    DAISY_PREP_LOOP(e, n) {
        if (e < n) keep[sval[e]] = (e == n - 1 || skey[e + 1] != skey[e]) ? kAlive : kDead;
    }
}

// DataFrame.query('rating >= t'): a NaN compares false and is dropped
__global__ __launch_bounds__(kBlock) void k_prep_threshold(const double *__restrict__ rating, double thr, int64_t n,
                                                           uint8_t *__restrict__ keep) {
    DAISY_PREP_LOOP(e, n) {
        if (e < n && !(rating[e] >= thr)) keep[e] = kDead;
    }
}

// The live rows of every id without an atomic: sorted[] holds the rows in the order of the first encoding's sort, so the
// rows of id r are the run [start[r], start[r + 1]); flag = the row is alive, excl = its exclusive scan.
__global__ __launch_bounds__(kBlock) void k_prep_live_flags(const int32_t *__restrict__ sorted, const uint8_t *__restrict__ keep,
                                                            int64_t n, uint32_t *__restrict__ flag) {
    DAISY_PREP_LOOP(e, n) {
        if (e < n) flag[e] = keep[sorted[e]] == kAlive ? 1u : 0u;
    }
}
__global__ __launch_bounds__(kBlock) void k_prep_run_counts(const uint32_t *__restrict__ start, int64_t space,
                                                            const uint32_t *__restrict__ flag, const uint32_t *__restrict__ excl,
                                                            int64_t n, int32_t *__restrict__ cnt) {
    DAISY_PREP_LOOP(r, space) {
        if (r < space) {
            const int64_t a = start[r], b = start[r + 1];
            const uint32_t upto = b == n ? excl[n - 1] + flag[n - 1] : excl[b];
            cnt[r] = (int32_t)(upto - excl[a]);
        }
    }
}

// N-filter, and N-core at level u or i: one pass against the counts of the frame as it stood (ucnt / icnt NULL: that
// side is not asked)
__global__ __launch_bounds__(kBlock) void k_prep_filter(const int32_t *__restrict__ u, const int32_t *__restrict__ i, int64_t n,
                                                        const int32_t *__restrict__ ucnt, const int32_t *__restrict__ icnt,
                                                        int32_t N, uint8_t *__restrict__ keep) {
    DAISY_PREP_LOOP(e, n) {
        if (e < n && keep[e] == kAlive && ((ucnt && ucnt[u[e]] < N) || (icnt && icnt[i[e]] < N))) keep[e] = kDead;
    }
}

// One round of the peel, first half: a live row whose user or item has fewer than N live rows is marked.  The counts
// are only read here, so every row of the round sees the counts the round began with (loader.py:268-269).
__global__ __launch_bounds__(kBlock) void k_prep_peel_mark(const int32_t *__restrict__ u, const int32_t *__restrict__ i, int64_t n,
                                                           const int32_t *__restrict__ ucnt, const int32_t *__restrict__ icnt,
                                                           int32_t N, uint8_t *__restrict__ keep, int32_t *__restrict__ changed) {
    DAISY_PREP_LOOP(e, n) {
        const bool dies = e < n && keep[e] == kAlive && (ucnt[u[e]] < N || icnt[i[e]] < N);
        if (dies) keep[e] = kDying;
        if (__ballot(dies) && threadIdx.x % kWave == 0) *changed = 1;
    }
}

// second half: the marked rows leave and take their counts with them (loader.py:280-284)
__global__ __launch_bounds__(kBlock) void k_prep_peel_apply(const int32_t *__restrict__ u, const int32_t *__restrict__ i, int64_t n,
                                                            int32_t *__restrict__ ucnt, int32_t *__restrict__ icnt,
                                                            uint8_t *__restrict__ keep) {
    DAISY_PREP_LOOP(e, n) {
        const bool dying = e < n && keep[e] == kDying;
        const int32_t uu = dying ? u[e] : 0, ii = dying ? i[e] : 0;
        if (dying) keep[e] = kDead;
        wave_count_add(ucnt, uu, dying, -1);
        wave_count_add(icnt, ii, dying, -1);
    }
}

__global__ __launch_bounds__(kBlock) void k_prep_keep_flags(const uint8_t *__restrict__ keep, int64_t n, uint32_t *__restrict__ flag) {
    DAISY_PREP_LOOP(e, n) {
        if (e < n) flag[e] = keep[e] == kAlive ? 1u : 0u;
    }
}

// the survivors in their original order; *total = their number
__global__ __launch_bounds__(kBlock) void k_prep_compact_rows(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ excl,
                                                              int64_t n, int32_t *__restrict__ rows, int64_t *__restrict__ total) {
    DAISY_PREP_LOOP(e, n) {
        if (e < n) {
            if (flag[e]) rows[excl[e]] = (int32_t)e;
            if (e == n - 1) *total = (int64_t)excl[e] + flag[e];
        }
    }
}

// __category_encoding: which first codes survive (every writer stores the same 1)
__global__ __launch_bounds__(kBlock) void k_prep_presence(const int32_t *__restrict__ c0, const int32_t *__restrict__ rows, int64_t m,
                                                          uint32_t *__restrict__ flag) {
    DAISY_PREP_LOOP(j, m) {
        if (j < m) flag[c0[rows[j]]] = 1u;
    }
}

__global__ __launch_bounds__(kBlock) void k_prep_recode(const int32_t *__restrict__ c0, const int32_t *__restrict__ rows, int64_t m,
                                                        const uint32_t *__restrict__ excl, int32_t *__restrict__ code) {
    DAISY_PREP_LOOP(j, m) {
        if (j < m) code[j] = (int32_t)excl[c0[rows[j]]];
    }
}

__global__ __launch_bounds__(kBlock) void k_prep_tokens(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ excl,
                                                        const int64_t *__restrict__ tok0, int64_t space, int64_t *__restrict__ tok,
                                                        const int32_t *__restrict__ cnt, int64_t user_num, double *__restrict__ pop,
                                                        int64_t *__restrict__ total) {
    DAISY_PREP_LOOP(c, space) {
        if (c < space) {
            if (flag[c]) {
                tok[excl[c]] = tok0[c];
                // loader.py:193: groupby(item).size() / user_num, one fp64 division of two integers
                if (pop) pop[excl[c]] = (double)cnt[c] / (double)user_num;
            }
            if (c == space - 1) *total = (int64_t)excl[c] + flag[c];
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_prep_time_keys(const int64_t *__restrict__ ts, const int32_t *__restrict__ rows, int64_t m,
                                                           uint64_t *__restrict__ key, int32_t *__restrict__ val) {
    DAISY_PREP_LOOP(j, m) {
        if (j < m) {
            key[j] = (uint64_t)ts[rows[j]] ^ kSignBit;
            val[j] = (int32_t)j;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_prep_emit(const int32_t *__restrict__ order, const int32_t *__restrict__ rows,
                                                      const int32_t *__restrict__ uc, const int32_t *__restrict__ ic, int64_t m,
                                                      int64_t *__restrict__ rows_out, int32_t *__restrict__ u_out,
                                                      int32_t *__restrict__ i_out) {
    DAISY_PREP_LOOP(p, m) {
        if (p < m) {
            const int32_t j = order[p];
            rows_out[p] = (int64_t)rows[j];
            u_out[p] = uc[j];
            i_out[p] = ic[j];
        }
    }
}

inline dim3 prep_grid(int64_t n) { return dim3(grid_for(n, kBlock)); }

// scratch that serves every u64-key sort of 1 .. n rows (a smaller sort may ask for more, see sort.hip) and every scan
inline size_t prep_temp_bytes(int64_t n) {
    size_t b = sort_pairs_u64_i32_temp_bytes(n);
    const size_t at_limit = sort_pairs_u64_i32_temp_bytes(n < 262144 ? n : 262144);
    if (at_limit > b) b = at_limit;
    const size_t sc = exclusive_scan_u32_temp_bytes(n);
    return b > sc ? b : sc;
}

struct PrepScratch {
    uint64_t *key_a, *key_b;
    int32_t *val_a, *val_b;
    uint32_t *flag, *excl;
    void *temp;
    size_t temp_bytes;
    int64_t *word;          // one device word the kernels report a total in
};

inline int read_word(const PrepScratch &sc, int64_t *out, hipStream_t s) {
    DAISY_HIP(hipMemcpyAsync(out, sc.word, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    DAISY_HIP(hipStreamSynchronize(s));
    return DAISY_OK;
}

// ids -> dense codes (the rank among the distinct values) and the distinct values ascending
// sorted / start (both or neither): the rows in sorted order and the run starts [distinct + 1], for live_counts
int encode_ids(const int64_t *ids, int64_t n, int32_t *codes, int64_t *tokens, int64_t *n_distinct, int32_t *sorted,
               uint32_t *start, const PrepScratch &sc, hipStream_t s) {
    int32_t *const sval = sorted ? sorted : sc.val_b;
    const dim3 g = prep_grid(n), b(kBlock);
    hipLaunchKernelGGL(k_prep_id_keys, g, b, 0, s, ids, n, sc.key_a, sc.val_a);
    DAISY_LAUNCH_CHECK();
    int rc = sort_pairs_u64_i32(sc.temp, sc.temp_bytes, sc.key_a, sc.key_b, sc.val_a, sval, n, 64, s);
    if (rc != DAISY_OK) return rc;
    hipLaunchKernelGGL(k_prep_run_heads, g, b, 0, s, sc.key_b, n, sc.flag);
    DAISY_LAUNCH_CHECK();
    rc = exclusive_scan_u32(sc.temp, sc.temp_bytes, sc.flag, sc.excl, n, s);
    if (rc != DAISY_OK) return rc;
    hipLaunchKernelGGL(k_prep_scatter_codes, g, b, 0, s, sc.key_b, sval, sc.flag, sc.excl, n, codes, tokens, start, sc.word);
    DAISY_LAUNCH_CHECK();
    return read_word(sc, n_distinct, s);
}

// cnt[r] = the live rows of id r, r < space
int live_counts(const int32_t *sorted, const uint32_t *start, int64_t space, const uint8_t *keep, int64_t n, int32_t *cnt,
                const PrepScratch &sc, hipStream_t s) {
    hipLaunchKernelGGL(k_prep_live_flags, prep_grid(n), dim3(kBlock), 0, s, sorted, keep, n, sc.flag);
    DAISY_LAUNCH_CHECK();
    const int rc = exclusive_scan_u32(sc.temp, sc.temp_bytes, sc.flag, sc.excl, n, s);
    if (rc != DAISY_OK) return rc;
    hipLaunchKernelGGL(k_prep_run_counts, prep_grid(space), dim3(kBlock), 0, s, start, space, sc.flag, sc.excl, n, cnt);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

// __category_encoding of one column: codes of the survivors, the surviving tokens, their number
// (cnt, user_num, pop: item_pop of the surviving items from their live counts; pop NULL: not asked)
int recode(const int32_t *c0, const int32_t *rows, int64_t m, int64_t space, const int64_t *tok0, int32_t *code, int64_t *tok,
           const int32_t *cnt, int64_t user_num, double *pop, int64_t *total, const PrepScratch &sc, hipStream_t s) {
    const dim3 b(kBlock);
    DAISY_HIP(hipMemsetAsync(sc.flag, 0, (size_t)space * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_prep_presence, prep_grid(m), b, 0, s, c0, rows, m, sc.flag);
    DAISY_LAUNCH_CHECK();
    const int rc = exclusive_scan_u32(sc.temp, sc.temp_bytes, sc.flag, sc.excl, space, s);
    if (rc != DAISY_OK) return rc;
    hipLaunchKernelGGL(k_prep_recode, prep_grid(m), b, 0, s, c0, rows, m, sc.excl, code);
    DAISY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_prep_tokens, prep_grid(space), b, 0, s, sc.flag, sc.excl, tok0, space, tok, cnt, user_num, pop, sc.word);
    DAISY_LAUNCH_CHECK();
    return read_word(sc, total, s);
}

void add_scratch(DeviceArena &arena, PrepScratch &sc, int64_t n) {
    arena.add(&sc.key_a, (size_t)n * sizeof(uint64_t));
    arena.add(&sc.key_b, (size_t)n * sizeof(uint64_t));
    arena.add(&sc.val_a, (size_t)n * sizeof(int32_t));
    arena.add(&sc.val_b, (size_t)n * sizeof(int32_t));
    arena.add(&sc.flag, (size_t)n * sizeof(uint32_t));
    arena.add(&sc.excl, (size_t)n * sizeof(uint32_t));
    sc.temp_bytes = prep_temp_bytes(n);
    arena.add(&sc.temp, sc.temp_bytes);
    arena.add(&sc.word, 4 * sizeof(int64_t));
}

struct ArenaGuard {         // the arena goes when the entry returns, on every path
    DeviceArena &a;
    ~ArenaGuard() { a.release(); }
};

}  // namespace
}  // namespace daisy

using namespace daisy;

extern "C" {

int daisy_prep_encode(const int64_t *ids, int64_t n, int32_t *codes, int64_t *tokens, int64_t *n_distinct_host,
                      daisy_stream_t stream) {
    DAISY_CHECK_ARG(ids && codes && tokens && n_distinct_host, "prep_encode: NULL argument");
    DAISY_CHECK_ARG(n >= 1 && n <= INT_MAX, "prep_encode: n=%lld outside [1, 2^31)", (long long)n);
    hipStream_t s = as_stream(stream);
    DeviceArena arena;
    PrepScratch sc;
    add_scratch(arena, sc, n);
    int rc = arena.alloc("prep_encode");
    if (rc != DAISY_OK) return rc;
    ArenaGuard guard{arena};
    return encode_ids(ids, n, codes, tokens, n_distinct_host, nullptr, nullptr, sc, s);
}

int daisy_prep_process(const int64_t *users, const int64_t *items, const double *rating, const int64_t *timestamp, int64_t n,
                       int32_t use_threshold, double threshold, int32_t mode, int32_t level, int32_t N, int32_t want_pop,
                       int64_t *rows, int32_t *user_code, int32_t *item_code, int64_t *uid_token, int64_t *iid_token,
                       double *item_pop, int64_t *stats_host, daisy_stream_t stream) {
    DAISY_CHECK_ARG(users && items && timestamp && rows && user_code && item_code && uid_token && iid_token && stats_host,
                    "prep_process: NULL argument");
    DAISY_CHECK_ARG(!use_threshold || rating, "prep_process: a threshold needs the ratings (NULL rating)");
    DAISY_CHECK_ARG(!want_pop || item_pop, "prep_process: NULL argument (item_pop)");
    DAISY_CHECK_ARG(n >= 1 && n <= INT_MAX, "prep_process: n=%lld outside [1, 2^31)", (long long)n);
    DAISY_CHECK_ARG(mode == DAISY_PREP_ORIGIN || mode == DAISY_PREP_FILTER || mode == DAISY_PREP_CORE,
                    "prep_process: mode=%d", mode);
    DAISY_CHECK_ARG(mode == DAISY_PREP_ORIGIN || (level >= 1 && level <= 3), "prep_process: level=%d (1 u, 2 i, 3 ui)", level);
    DAISY_CHECK_ARG(mode == DAISY_PREP_ORIGIN || N >= 1, "prep_process: N=%d, must be >= 1", N);
    hipStream_t s = as_stream(stream);

    DeviceArena arena;
    PrepScratch sc;
    int32_t *c0u, *c0i, *live, *uc, *ic, *ucnt, *icnt, *changed, *by_user, *by_item;
    uint32_t *ustart, *istart;
    int64_t *tok0u, *tok0i;
    uint8_t *keep;
    add_scratch(arena, sc, n);
    arena.add(&c0u, (size_t)n * sizeof(int32_t));
    arena.add(&c0i, (size_t)n * sizeof(int32_t));
    arena.add(&tok0u, (size_t)n * sizeof(int64_t));
    arena.add(&tok0i, (size_t)n * sizeof(int64_t));
    arena.add(&live, (size_t)n * sizeof(int32_t));
    arena.add(&uc, (size_t)n * sizeof(int32_t));
    arena.add(&ic, (size_t)n * sizeof(int32_t));
    arena.add(&ucnt, (size_t)n * sizeof(int32_t));
    arena.add(&icnt, (size_t)n * sizeof(int32_t));
    arena.add(&by_user, (size_t)n * sizeof(int32_t));
    arena.add(&by_item, (size_t)n * sizeof(int32_t));
    arena.add(&ustart, (size_t)(n + 1) * sizeof(uint32_t));
    arena.add(&istart, (size_t)(n + 1) * sizeof(uint32_t));
    arena.add(&keep, (size_t)n);
    arena.add(&changed, sizeof(int32_t));
    int rc = arena.alloc("prep_process");
    if (rc != DAISY_OK) return rc;
    ArenaGuard guard{arena};

    const dim3 g = prep_grid(n), b(kBlock);
    // (a) first encoding
    int64_t U0 = 0, I0 = 0;
    if ((rc = encode_ids(users, n, c0u, tok0u, &U0, by_user, ustart, sc, s)) != DAISY_OK) return rc;
    if ((rc = encode_ids(items, n, c0i, tok0i, &I0, by_item, istart, sc, s)) != DAISY_OK) return rc;
    // (b) drop_duplicates([user, item], keep='last')
    hipLaunchKernelGGL(k_prep_pair_keys, g, b, 0, s, c0u, c0i, n, sc.key_a, sc.val_a);
    DAISY_LAUNCH_CHECK();
    if ((rc = sort_pairs_u64_i32(sc.temp, sc.temp_bytes, sc.key_a, sc.key_b, sc.val_a, sc.val_b, n, 32 + bits_for(U0), s)) !=
        DAISY_OK)
        return rc;
    hipLaunchKernelGGL(k_prep_mark_last, g, b, 0, s, sc.key_b, sc.val_b, n, keep);
    DAISY_LAUNCH_CHECK();
    // (c) rating >= positive_threshold
    if (use_threshold) {
        hipLaunchKernelGGL(k_prep_threshold, g, b, 0, s, rating, threshold, n, keep);
        DAISY_LAUNCH_CHECK();
    }
    // (d) core filter
    int64_t rounds = 0;
    if (mode != DAISY_PREP_ORIGIN) {
        const bool peel = mode == DAISY_PREP_CORE && level == 3;
        int32_t *const uside = (level & 1) ? ucnt : nullptr, *const iside = (level & 2) ? icnt : nullptr;
        if (uside && (rc = live_counts(by_user, ustart, U0, keep, n, ucnt, sc, s)) != DAISY_OK) return rc;
        if (iside && (rc = live_counts(by_item, istart, I0, keep, n, icnt, sc, s)) != DAISY_OK) return rc;
        if (!peel) {
            hipLaunchKernelGGL(k_prep_filter, g, b, 0, s, c0u, c0i, n, uside, iside, N, keep);
            DAISY_LAUNCH_CHECK();
        } else {
            for (;;) {          // at most n rounds: every round but the last removes a row
                DAISY_HIP(hipMemsetAsync(changed, 0, sizeof(int32_t), s));
                hipLaunchKernelGGL(k_prep_peel_mark, g, b, 0, s, c0u, c0i, n, ucnt, icnt, N, keep, changed);
                DAISY_LAUNCH_CHECK();
                int32_t any = 0;
                DAISY_HIP(hipMemcpyAsync(&any, changed, sizeof(int32_t), hipMemcpyDeviceToHost, s));
                DAISY_HIP(hipStreamSynchronize(s));
                if (!any) break;
                hipLaunchKernelGGL(k_prep_peel_apply, g, b, 0, s, c0u, c0i, n, ucnt, icnt, keep);
                DAISY_LAUNCH_CHECK();
                ++rounds;
            }
        }
    }
    // the survivors in their order
    int64_t m = 0;
    hipLaunchKernelGGL(k_prep_keep_flags, g, b, 0, s, keep, n, sc.flag);
    DAISY_LAUNCH_CHECK();
    if ((rc = exclusive_scan_u32(sc.temp, sc.temp_bytes, sc.flag, sc.excl, n, s)) != DAISY_OK) return rc;
    hipLaunchKernelGGL(k_prep_compact_rows, g, b, 0, s, sc.flag, sc.excl, n, live, sc.word);
    DAISY_LAUNCH_CHECK();
    if ((rc = read_word(sc, &m, s)) != DAISY_OK) return rc;
    stats_host[0] = m;
    stats_host[1] = stats_host[2] = 0;
    stats_host[3] = rounds;
    if (m == 0) return DAISY_OK;
    // (e) final encoding, and (g) item_pop from the survivors' counts per item
    int64_t user_num = 0, item_num = 0;
    if (want_pop && (rc = live_counts(by_item, istart, I0, keep, n, icnt, sc, s)) != DAISY_OK) return rc;
    if ((rc = recode(c0u, live, m, U0, tok0u, uc, uid_token, nullptr, 0, nullptr, &user_num, sc, s)) != DAISY_OK) return rc;
    if ((rc = recode(c0i, live, m, I0, tok0i, ic, iid_token, icnt, user_num, want_pop ? item_pop : nullptr, &item_num, sc, s)) !=
        DAISY_OK)
        return rc;
    stats_host[1] = user_num;
    stats_host[2] = item_num;
    // (f) stable sort by timestamp
    const dim3 gm = prep_grid(m);
    hipLaunchKernelGGL(k_prep_time_keys, gm, b, 0, s, timestamp, live, m, sc.key_a, sc.val_a);
    DAISY_LAUNCH_CHECK();
    if ((rc = sort_pairs_u64_i32(sc.temp, sc.temp_bytes, sc.key_a, sc.key_b, sc.val_a, sc.val_b, m, 64, s)) != DAISY_OK) return rc;
    hipLaunchKernelGGL(k_prep_emit, gm, b, 0, s, sc.val_b, live, uc, ic, m, rows, user_code, item_code);
    DAISY_LAUNCH_CHECK();
    DAISY_HIP(hipStreamSynchronize(s));     // the arena is released on return
    return DAISY_OK;
}

}  // extern "C"
