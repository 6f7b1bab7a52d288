// split_test / split_validation (daisy/utils/splitter.py:29-185) on the device, for any frame: the user
// column arrives as dense codes (daisy_prep_encode).  tloo is two integer-atomic passes (max of an order-preserving key,
// then min row among its holders); utfo, ufo and rloo group the rows by user with a stable sort and take a head or a tail
// of every group; the random methods order the rows by a Philox key of (seed, fold, row) first.  Integer atomics only
// (max and min do not depend on their order): two calls give identical ids.
#include <limits.h>
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace daisy {
namespace {

constexpr uint64_t kSignBit = 1ull << 63;
constexpr uint64_t kSplitStream = 1ull << 59;       // Philox stream of fold f: kSplitStream | f

#define DAISY_SPLIT_LOOP(e, n)                                                                                    \
    for (int64_t e = blockIdx.x * (int64_t)kBlock + threadIdx.x; e < (n); e += (int64_t)gridDim.x * kBlock)

__global__ __launch_bounds__(kBlock) void k_split_iota(int64_t n, int32_t *__restrict__ val) {
    DAISY_SPLIT_LOOP(e, n) val[e] = (int32_t)e;
}

__global__ __launch_bounds__(kBlock) void k_split_rand_keys(int64_t n, uint64_t seed, uint64_t stream,
                                                            uint64_t *__restrict__ key, int32_t *__restrict__ val) {
    DAISY_SPLIT_LOOP(e, n) {
        key[e] = philox_u64(seed, stream, (uint64_t)e);
        val[e] = (int32_t)e;
    }
}

__global__ __launch_bounds__(kBlock) void k_split_gather_group(const int32_t *__restrict__ ucode, const int32_t *__restrict__ val,
                                                               int64_t n, int32_t *__restrict__ gk) {
    DAISY_SPLIT_LOOP(e, n) gk[e] = ucode[val[e]];
}

// [start, end) of every user's run in the grouped order
// (a code outside [0, U) owns no run: its rows stay in train)
__global__ __launch_bounds__(kBlock) void k_split_bounds(const int32_t *__restrict__ sgk, int64_t n, int64_t U,
                                                         int32_t *__restrict__ start, int32_t *__restrict__ end) {
    DAISY_SPLIT_LOOP(e, n) {
        const int32_t u = sgk[e];
        if (u < 0 || u >= U) continue;
        if (e == 0 || sgk[e - 1] != u) start[u] = (int32_t)e;
        if (e == n - 1 || sgk[e + 1] != u) end[u] = (int32_t)(e + 1);
    }
}

// utfo: the rows after the first ceil(len * (1 - size)) (splitter.py:61); ufo: the first round(len * size) in key order
// (DataFrame.sample(frac): round half to even, so rint); rloo: the first one.  Both products are the reference's fp64
// expressions, hence its counts.
__global__ __launch_bounds__(kBlock) void k_split_mark_groups(int32_t method, const int32_t *__restrict__ sgk,
                                                              const int32_t *__restrict__ sval, int64_t n, int64_t U,
                                                              const int32_t *__restrict__ start, const int32_t *__restrict__ end,
                                                              double size, double one_minus, uint32_t *__restrict__ mask_sorted,
                                                              uint32_t *__restrict__ mask_row) {
    DAISY_SPLIT_LOOP(e, n) {
        const int32_t u = sgk[e];
        const bool in = u >= 0 && u < U;
        const int64_t pos = in ? e - start[u] : 0, len = in ? (int64_t)end[u] - start[u] : 0;
        bool test;
        if (!in) test = false;
        else if (method == DAISY_SPLIT_UTFO) test = pos >= (int64_t)ceil((double)len * one_minus);
        else if (method == DAISY_SPLIT_UFO) test = pos < (int64_t)rint((double)len * size);
        else test = pos == 0;
        mask_sorted[e] = test ? 1u : 0u;
        mask_row[sval[e]] = test ? 1u : 0u;
    }
}

__global__ __launch_bounds__(kBlock) void k_split_mark_head(const int32_t *__restrict__ sval, int64_t n, int64_t head,
                                                            uint32_t *__restrict__ mask_sorted, uint32_t *__restrict__ mask_row) {
    DAISY_SPLIT_LOOP(e, n) {
        mask_sorted[e] = e < head ? 1u : 0u;
        mask_row[sval[e]] = e < head ? 1u : 0u;
    }
}

// tloo, pass 1: the largest timestamp of every user.  The table only grows, so a value already reached needs no atomic.
__global__ __launch_bounds__(kBlock) void k_split_tloo_max(const int32_t *__restrict__ ucode, const int64_t *__restrict__ ts, int64_t n,
                                                           int64_t U, unsigned long long *__restrict__ best) {
    DAISY_SPLIT_LOOP(e, n) {
        if (ucode[e] < 0 || ucode[e] >= U) continue;
        const unsigned long long k = (unsigned long long)((uint64_t)ts[e] ^ kSignBit);
        unsigned long long *p = best + ucode[e];
        if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < k) atomicMax(p, k);
    }
}
// pass 2: the earliest row that holds it (rank(method='first', ascending=False) == 1, splitter.py:80)
__global__ __launch_bounds__(kBlock) void k_split_tloo_min(const int32_t *__restrict__ ucode, const int64_t *__restrict__ ts, int64_t n,
                                                           int64_t U, const unsigned long long *__restrict__ best,
                                                           unsigned int *__restrict__ first) {
    DAISY_SPLIT_LOOP(e, n) {
        const int32_t u = ucode[e];
        if (u < 0 || u >= U) continue;
        if ((unsigned long long)((uint64_t)ts[e] ^ kSignBit) != best[u]) continue;
        unsigned int *p = first + u;
        if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (unsigned int)e) atomicMin(p, (unsigned int)e);
    }
}
__global__ __launch_bounds__(kBlock) void k_split_tloo_mark(const int32_t *__restrict__ ucode, int64_t n, int64_t U,
                                                            const unsigned int *__restrict__ first, uint32_t *__restrict__ mask_row) {
    DAISY_SPLIT_LOOP(e, n) {
        const int32_t u = ucode[e];
        mask_row[e] = (u >= 0 && u < U && first[u] == (unsigned int)e) ? 1u : 0u;
    }
}

// out = the ids whose flag equals `want`, in the order of e (src NULL: the id is e itself); *total = their number
__global__ __launch_bounds__(kBlock) void k_split_compact(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ excl,
                                                          const int32_t *__restrict__ src, int64_t n, uint32_t want,
                                                          int64_t *__restrict__ out, int64_t *__restrict__ total) {
    DAISY_SPLIT_LOOP(e, n) {
        const int64_t ones = excl[e];                                   // flags set before e
        const int64_t at = want ? ones : e - ones;
        if (flag[e] == want) out[at] = src ? (int64_t)src[e] : e;
        if (e == n - 1) *total = at + (flag[e] == want ? 1 : 0);
    }
}

inline size_t split_temp_bytes(int64_t n) {
    size_t b = sort_pairs_u64_i32_temp_bytes(n);
    const size_t at_limit = sort_pairs_u64_i32_temp_bytes(n < 262144 ? n : 262144);
    if (at_limit > b) b = at_limit;
    const size_t b32 = sort_pairs_i32_temp_bytes_upto(n), sc = exclusive_scan_u32_temp_bytes(n);
    if (b32 > b) b = b32;
    return b > sc ? b : sc;
}

struct ArenaGuard {
    DeviceArena &a;
    ~ArenaGuard() { a.release(); }
};

}  // namespace
}  // namespace daisy

using namespace daisy;

extern "C" {

int daisy_split_ids(int32_t method, const int32_t *user_code, const int64_t *timestamp, int64_t n, int64_t user_num, double size,
                    double one_minus_size, uint64_t seed, uint64_t fold, int64_t *train, int64_t *test, int64_t *counts_host,
                    daisy_stream_t stream) {
    DAISY_CHECK_ARG(method >= DAISY_SPLIT_TLOO && method <= DAISY_SPLIT_RSBR, "split_ids: method=%d", method);
    DAISY_CHECK_ARG(train && test && counts_host, "split_ids: NULL argument");
    DAISY_CHECK_ARG(method == DAISY_SPLIT_RSBR || user_code, "split_ids: NULL argument (user_code)");
    DAISY_CHECK_ARG(method != DAISY_SPLIT_TLOO || timestamp, "split_ids: tloo needs the timestamps (NULL timestamp)");
    DAISY_CHECK_ARG(n >= 1 && n <= INT_MAX, "split_ids: n=%lld outside [1, 2^31)", (long long)n);
    DAISY_CHECK_ARG(method == DAISY_SPLIT_RSBR || (user_num >= 1 && user_num <= n), "split_ids: user_num=%lld outside [1, n=%lld]",
                    (long long)user_num, (long long)n);
    const bool sized = method == DAISY_SPLIT_UTFO || method == DAISY_SPLIT_UFO || method == DAISY_SPLIT_RSBR;
    DAISY_CHECK_ARG(!sized || (size > 0.0 && size < 1.0), "split_ids: size=%g outside (0, 1)", size);
    hipStream_t s = as_stream(stream);
    const int64_t U = method == DAISY_SPLIT_RSBR ? 1 : user_num;

    DeviceArena arena;
    uint64_t *key_a, *key_b;
    int32_t *val_a, *val_b, *val_c, *gk_a, *gk_b, *start, *end;
    unsigned long long *best;
    unsigned int *first;
    uint32_t *mask_sorted, *mask_row, *excl;
    int64_t *word;
    void *temp;
    const size_t temp_bytes = split_temp_bytes(n);
    arena.add(&key_a, (size_t)n * sizeof(uint64_t));
    arena.add(&key_b, (size_t)n * sizeof(uint64_t));
    arena.add(&val_a, (size_t)n * sizeof(int32_t));
    arena.add(&val_b, (size_t)n * sizeof(int32_t));
    arena.add(&val_c, (size_t)n * sizeof(int32_t));
    arena.add(&gk_a, (size_t)n * sizeof(int32_t));
    arena.add(&gk_b, (size_t)n * sizeof(int32_t));
    arena.add(&start, (size_t)U * sizeof(int32_t));
    arena.add(&end, (size_t)U * sizeof(int32_t));
    arena.add(&best, (size_t)U * sizeof(unsigned long long));
    arena.add(&first, (size_t)U * sizeof(unsigned int));
    arena.add(&mask_sorted, (size_t)n * sizeof(uint32_t));
    arena.add(&mask_row, (size_t)n * sizeof(uint32_t));
    arena.add(&excl, (size_t)n * sizeof(uint32_t));
    arena.add(&word, 2 * sizeof(int64_t));
    arena.add(&temp, temp_bytes);
    int rc = arena.alloc("split_ids");
    if (rc != DAISY_OK) return rc;
    ArenaGuard guard{arena};

    const dim3 g(grid_for(n, kBlock)), b(kBlock);
    const int32_t *order = nullptr;                 // the grouped order the test ids come out in; NULL: row order
    if (method == DAISY_SPLIT_TLOO) {
        DAISY_HIP(hipMemsetAsync(best, 0, (size_t)U * sizeof(unsigned long long), s));
        DAISY_HIP(hipMemsetAsync(first, 0xFF, (size_t)U * sizeof(unsigned int), s));
        hipLaunchKernelGGL(k_split_tloo_max, g, b, 0, s, user_code, timestamp, n, U, best);
        DAISY_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_split_tloo_min, g, b, 0, s, user_code, timestamp, n, U, best, first);
        DAISY_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_split_tloo_mark, g, b, 0, s, user_code, n, U, first, mask_row);
        DAISY_LAUNCH_CHECK();
    } else {
        const int32_t *rows_in;                     // the rows in key order (random methods) or row order (utfo)
        if (method == DAISY_SPLIT_UTFO) {
            hipLaunchKernelGGL(k_split_iota, g, b, 0, s, n, val_a);
            DAISY_LAUNCH_CHECK();
            rows_in = val_a;
        } else {
            hipLaunchKernelGGL(k_split_rand_keys, g, b, 0, s, n, seed, kSplitStream | fold, key_a, val_a);
            DAISY_LAUNCH_CHECK();
            if ((rc = sort_pairs_u64_i32(temp, temp_bytes, key_a, key_b, val_a, val_b, n, 64, s)) != DAISY_OK) return rc;
            rows_in = val_b;
        }
        if (method == DAISY_SPLIT_RSBR) {
            const int64_t head = (int64_t)((double)n * size);           // splitter.py:76: int(len(df) * test_size)
            hipLaunchKernelGGL(k_split_mark_head, g, b, 0, s, rows_in, n, head, mask_sorted, mask_row);
            DAISY_LAUNCH_CHECK();
            order = rows_in;
        } else {
            hipLaunchKernelGGL(k_split_gather_group, g, b, 0, s, user_code, rows_in, n, gk_a);
            DAISY_LAUNCH_CHECK();
            if ((rc = sort_pairs_i32(temp, temp_bytes, gk_a, gk_b, rows_in, val_c, n, bits_for(U), s)) != DAISY_OK) return rc;
            DAISY_HIP(hipMemsetAsync(start, 0, (size_t)U * sizeof(int32_t), s));
            DAISY_HIP(hipMemsetAsync(end, 0, (size_t)U * sizeof(int32_t), s));
            hipLaunchKernelGGL(k_split_bounds, g, b, 0, s, gk_b, n, U, start, end);
            DAISY_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_split_mark_groups, g, b, 0, s, method, gk_b, val_c, n, U, start, end, size, one_minus_size,
                               mask_sorted, mask_row);
            DAISY_LAUNCH_CHECK();
            order = val_c;
        }
    }
    // test: the marked rows in the grouped order (tloo: in row order); train: the others, ascending
    const uint32_t *test_flags = order ? mask_sorted : mask_row;
    if ((rc = exclusive_scan_u32(temp, temp_bytes, test_flags, excl, n, s)) != DAISY_OK) return rc;
    hipLaunchKernelGGL(k_split_compact, g, b, 0, s, test_flags, excl, order, n, 1u, test, word + 1);
    DAISY_LAUNCH_CHECK();
    if (order && (rc = exclusive_scan_u32(temp, temp_bytes, mask_row, excl, n, s)) != DAISY_OK) return rc;
    hipLaunchKernelGGL(k_split_compact, g, b, 0, s, mask_row, excl, (const int32_t *)nullptr, n, 0u, train, word);
    DAISY_LAUNCH_CHECK();
    DAISY_HIP(hipMemcpyAsync(counts_host, word, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    DAISY_HIP(hipStreamSynchronize(s));
    return DAISY_OK;
}

}  // extern "C"
