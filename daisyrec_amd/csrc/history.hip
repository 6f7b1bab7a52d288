// get_history_matrix (daisy/utils/utils.py:87-123), the CSR its padded pair stands for under index_put_ without
// accumulation (AbstractRecommender.py:147-158) and pandas.unique's first-seen order (dataset.py:52) on the device;
// DESIGN.md §23.  Everything is integer work apart from one double -> float cast per value: the sorts and scans are
// sort.hip's rocPRIM wrappers (stable radix sorts told their key width), the kernels around them are below.  The order
// inside a row comes from the stable sort, never from an atomic; the only atomics are an integer max (the longest row)
// and an integer min (the first position of an id), whose results do not depend on their order, so two calls give
// identical bytes.
#include <limits.h>

#include "common.h"

namespace daisy {
namespace {

// the elements of a grid-stride loop whose trip count is the same for every lane of a workgroup
#define DAISY_HIST_LOOP(e, n)                                                                                     \
    for (int64_t base_ = blockIdx.x * (int64_t)kBlock; base_ < (n); base_ += (int64_t)gridDim.x * kBlock)        \
        if (const int64_t e = base_ + threadIdx.x; true)

constexpr int kFillPerLane = 4;                         // cells per lane and trip of the padded fill
constexpr int kFillTile = kBlock * kFillPerLane;

__global__ __launch_bounds__(kBlock) void k_hist_row_keys(const int32_t *__restrict__ row, int64_t n, int32_t *__restrict__ key,
                                                          int32_t *__restrict__ val) {
    DAISY_HIST_LOOP(e, n) {
        if (e < n) {
            key[e] = row[e];
            val[e] = (int32_t)e;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_hist_pair_keys(const int32_t *__restrict__ row, const int32_t *__restrict__ col,
                                                           int64_t n, int col_bits, uint64_t *__restrict__ key,
                                                           int32_t *__restrict__ val) {
    DAISY_HIST_LOOP(e, n) {
        if (e < n) {
            // row above the column's bits: the kernels behind the sort read both back from the key instead of gathering
            key[e] = ((uint64_t)(uint32_t)row[e] << col_bits) | (uint64_t)(uint32_t)col[e];
            val[e] = (int32_t)e;
        }
    }
}

// start[r] = the first sorted entry whose key is >= r << shift, r <= row_num (absent rows get an empty range): a binary
// search per row, so a frame without some rows (a validation fold) costs nothing extra
template <class K, class S>
__global__ __launch_bounds__(kBlock) void k_hist_row_starts(const K *__restrict__ skey, int64_t n, int64_t row_num, int shift,
                                                            S *__restrict__ start) {
    DAISY_HIST_LOOP(r, row_num + 1) {
        if (r <= row_num) {
            const uint64_t want = (uint64_t)r << shift;
            int64_t lo = 0, hi = n;
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if ((uint64_t)skey[mid] < want) lo = mid + 1;
                else hi = mid;
            }
            start[r] = (S)lo;
        }
    }
}

// len[r] (NULL: not asked) and the longest row: a maximum per wave, one integer atomicMax per wave
template <class S>
__global__ __launch_bounds__(kBlock) void k_hist_lens(const S *__restrict__ start, int64_t row_num, int64_t *__restrict__ len,
                                                      unsigned long long *__restrict__ longest) {
    DAISY_HIST_LOOP(r, row_num) {
        int32_t m = 0;
        if (r < row_num) {
            m = (int32_t)(start[r + 1] - start[r]);
            if (len) len[r] = (int64_t)m;
        }
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {
            const int32_t o = __shfl_xor(m, off, kWave);
            m = o > m ? o : m;
        }
        if (threadIdx.x % kWave == 0 && m > 0) atomicMax(longest, (unsigned long long)m);
    }
}

// Every cell of the padded pair exactly once, in cell order (coalesced 8- and 4-byte stores): cell (r, p) is the sorted
// entry start[r] + p when p < len[r], zero otherwise.  A workgroup's tile begins at cell base = r0 * L + p0; r0 and p0
// advance with the loop (two 64-bit divisions per workgroup, none per trip), and a lane's cell is a 32-bit division
// away: p0 + lane offset < L + kFillTile < 2^32.
__global__ __launch_bounds__(kBlock) void k_hist_fill(const int32_t *__restrict__ order, const int64_t *__restrict__ start,
                                                      const int32_t *__restrict__ col, const double *__restrict__ val,
                                                      int64_t L, int64_t cells, int64_t *__restrict__ hid,
                                                      float *__restrict__ hval) {
    const int64_t stride = (int64_t)gridDim.x * kFillTile;
    const int64_t sr = stride / L, sp = stride - sr * L;
    int64_t base = blockIdx.x * (int64_t)kFillTile;
    int64_t r0 = base / L, p0 = base - r0 * L;
    const uint32_t Lu = (uint32_t)L;
    for (; base < cells; base += stride) {
#pragma unroll
        for (int k = 0; k < kFillPerLane; ++k) {
            const uint32_t off = (uint32_t)p0 + (uint32_t)(k * kBlock) + threadIdx.x;
            const int64_t c = base + k * kBlock + threadIdx.x;
            if (c < cells) {
                const uint32_t dr = off / Lu, p = off - dr * Lu;
                const int64_t r = r0 + dr;                       // c < cells = row_num * L, so r < row_num
                const int64_t a = start[r], len = start[r + 1] - a;
                int64_t id = 0;
                float v = 0.f;
                if ((int64_t)p < len) {
                    const int32_t e = order[a + p];
                    id = (int64_t)col[e];
                    v = val ? (float)val[e] : 1.f;
                }
                hid[c] = id;
                hval[c] = v;
            }
        }
        r0 += sr;
        p0 += sp;
        if (p0 >= L) {
            p0 -= L;
            ++r0;
        }
    }
}

// index_put_ without accumulation, entry by entry of the (row, col)-sorted frame: the tail of a run of equal pairs is
// its last frame position (the sort is stable and the positions went in ascending) and the write that stays; a row
// shorter than the longest has its column 0 overwritten by the padding (0, 0.0); a value that is 0 in fp32 adds nothing.
// Row and column come out of the key; the value is the one gather, and only the tail of a run pays for it.
__global__ __launch_bounds__(kBlock) void k_hist_csr_flags(const uint64_t *__restrict__ skey, const int32_t *__restrict__ sval,
                                                           const double *__restrict__ val, const uint32_t *__restrict__ start,
                                                           const unsigned long long *__restrict__ longest, int64_t n,
                                                           int col_bits, uint32_t *__restrict__ flag) {
    const uint32_t L = (uint32_t)*longest;
    const uint64_t col_mask = ((uint64_t)1 << col_bits) - 1;
    DAISY_HIST_LOOP(e, n) {
        if (e < n) {
            const uint64_t k = skey[e];
            bool keep = e == n - 1 || skey[e + 1] != k;
            if (keep && (k & col_mask) == 0) {
                const uint64_t r = k >> col_bits;
                keep = start[r + 1] - start[r] >= L;
            }
            if (keep && val) keep = (float)val[sval[e]] != 0.f;
            flag[e] = keep ? 1u : 0u;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_hist_csr_emit(const uint64_t *__restrict__ skey, const int32_t *__restrict__ sval,
                                                          const uint32_t *__restrict__ flag, const uint32_t *__restrict__ excl,
                                                          const double *__restrict__ val, int64_t n, int col_bits,
                                                          int32_t *__restrict__ out_col, float *__restrict__ out_val,
                                                          int64_t *__restrict__ total) {
    const uint64_t col_mask = ((uint64_t)1 << col_bits) - 1;
    DAISY_HIST_LOOP(e, n) {
        if (e < n) {
            if (flag[e]) {
                out_col[excl[e]] = (int32_t)(skey[e] & col_mask);
                out_val[excl[e]] = val ? (float)val[sval[e]] : 1.f;
            }
            if (e == n - 1) *total = (int64_t)excl[e] + flag[e];
        }
    }
}

// row_ptr[r] = the kept entries before row r's first sorted entry
__global__ __launch_bounds__(kBlock) void k_hist_row_ptr(const uint32_t *__restrict__ start, const uint32_t *__restrict__ flag,
                                                         const uint32_t *__restrict__ excl, int64_t n, int64_t row_num,
                                                         int64_t *__restrict__ row_ptr) {
    DAISY_HIST_LOOP(r, row_num + 1) {
        if (r <= row_num) {
            const int64_t s = start[r];
            row_ptr[r] = s == n ? (int64_t)excl[n - 1] + flag[n - 1] : (int64_t)excl[s];
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_hist_fill_i32(int32_t *__restrict__ x, int64_t n, int32_t v) {
    DAISY_HIST_LOOP(e, n) {
        if (e < n) x[e] = v;
    }
}

// first[id] = the smallest frame position that holds id.  A hot id is read before it is contended for: the value only
// ever falls, so a stale read costs one atomic and never a wrong result.
__global__ __launch_bounds__(kBlock) void k_hist_first_min(const int32_t *__restrict__ ids, int64_t n, int32_t *__restrict__ first) {
    DAISY_HIST_LOOP(e, n) {
        if (e < n) {
            int32_t *const slot = first + ids[e];
            if ((int32_t)e < __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(slot, (int32_t)e);
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_hist_head_flags(const int32_t *__restrict__ ids, const int32_t *__restrict__ first,
                                                            int64_t n, uint32_t *__restrict__ flag) {
    DAISY_HIST_LOOP(e, n) {
        if (e < n) flag[e] = first[ids[e]] == (int32_t)e ? 1u : 0u;
    }
}

__global__ __launch_bounds__(kBlock) void k_hist_first_emit(const int32_t *__restrict__ ids, const uint32_t *__restrict__ flag,
                                                            const uint32_t *__restrict__ excl, int64_t n, int64_t *__restrict__ out,
                                                            int64_t *__restrict__ total) {
    DAISY_HIST_LOOP(e, n) {
        if (e < n) {
            if (flag[e]) out[excl[e]] = (int64_t)ids[e];
            if (e == n - 1) *total = (int64_t)excl[e] + flag[e];
        }
    }
}

inline dim3 hist_grid(int64_t n) { return dim3(grid_for(n, kBlock)); }

// scratch that serves the u64-key sort of 1 .. n rows (a smaller sort may ask for more, see sort.hip) and every scan
inline size_t pair_temp_bytes(int64_t n) {
    size_t b = sort_pairs_u64_i32_temp_bytes(n);
    const size_t at_limit = sort_pairs_u64_i32_temp_bytes(n < 262144 ? n : 262144);
    if (at_limit > b) b = at_limit;
    const size_t sc = exclusive_scan_u32_temp_bytes(n);
    return b > sc ? b : sc;
}

struct ArenaGuard {         // the arena goes when the entry returns, on every path
    DeviceArena &a;
    ~ArenaGuard() { a.release(); }
};

inline bool dim_ok(int64_t x) { return x >= 1 && x <= INT_MAX; }

}  // namespace
}  // namespace daisy

using namespace daisy;

extern "C" {

int daisy_history_counts(const int32_t *row, int64_t n, int64_t row_num, int32_t *order, int64_t *start,
                         int64_t *history_len, int64_t *longest_host, daisy_stream_t stream) {
    DAISY_CHECK_ARG(row && order && start && history_len && longest_host, "history_counts: NULL argument");
    DAISY_CHECK_ARG(dim_ok(n), "history_counts: n=%lld outside [1, 2^31)", (long long)n);
    DAISY_CHECK_ARG(dim_ok(row_num), "history_counts: row_num=%lld outside [1, 2^31)", (long long)row_num);
    hipStream_t s = as_stream(stream);
    DeviceArena arena;
    int32_t *key_a, *key_b, *val_a;
    void *temp;
    unsigned long long *word;
    const size_t temp_bytes = sort_pairs_i32_temp_bytes_upto(n);
    arena.add(&key_a, (size_t)n * sizeof(int32_t));
    arena.add(&key_b, (size_t)n * sizeof(int32_t));
    arena.add(&val_a, (size_t)n * sizeof(int32_t));
    arena.add(&temp, temp_bytes);
    arena.add(&word, sizeof(unsigned long long));
    int rc = arena.alloc("history_counts");
    if (rc != DAISY_OK) return rc;
    ArenaGuard guard{arena};

    const dim3 b(kBlock);
    hipLaunchKernelGGL(k_hist_row_keys, hist_grid(n), b, 0, s, row, n, key_a, val_a);
    DAISY_LAUNCH_CHECK();
    if ((rc = sort_pairs_i32(temp, temp_bytes, key_a, key_b, val_a, order, n, bits_for(row_num), s)) != DAISY_OK) return rc;
    hipLaunchKernelGGL((k_hist_row_starts<int32_t, int64_t>), hist_grid(row_num + 1), b, 0, s, key_b, n, row_num, 0, start);
    DAISY_LAUNCH_CHECK();
    DAISY_HIP(hipMemsetAsync(word, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL((k_hist_lens<int64_t>), hist_grid(row_num), b, 0, s, start, row_num, history_len, word);
    DAISY_LAUNCH_CHECK();
    unsigned long long longest = 0;
    DAISY_HIP(hipMemcpyAsync(&longest, word, sizeof(longest), hipMemcpyDeviceToHost, s));
    DAISY_HIP(hipStreamSynchronize(s));
    *longest_host = (int64_t)longest;
    return DAISY_OK;
}

int daisy_history_fill(const int32_t *order, const int64_t *start, const int32_t *col, const double *val, int64_t n,
                       int64_t row_num, int64_t L, int64_t *history_matrix, float *history_value, daisy_stream_t stream) {
    DAISY_CHECK_ARG(order && start && col && history_matrix && history_value, "history_fill: NULL argument");
    DAISY_CHECK_ARG(dim_ok(n), "history_fill: n=%lld outside [1, 2^31)", (long long)n);
    DAISY_CHECK_ARG(dim_ok(row_num), "history_fill: row_num=%lld outside [1, 2^31)", (long long)row_num);
    DAISY_CHECK_ARG(L >= 1 && L <= n, "history_fill: L=%lld outside [1, n]", (long long)L);
    hipStream_t s = as_stream(stream);
    const int64_t cells = row_num * L;
    hipLaunchKernelGGL(k_hist_fill, dim3(grid_for(cells, kFillTile)), dim3(kBlock), 0, s, order, start, col, val, L, cells,
                       history_matrix, history_value);
    DAISY_LAUNCH_CHECK();
    DAISY_HIP(hipStreamSynchronize(s));
    return DAISY_OK;
}

int daisy_history_csr(const int32_t *row, const int32_t *col, const double *val, int64_t n, int64_t row_num, int64_t col_num,
                      int64_t *row_ptr, int32_t *out_col, float *out_val, int64_t *totals_host, daisy_stream_t stream) {
    DAISY_CHECK_ARG(row && col && row_ptr && out_col && out_val && totals_host, "history_csr: NULL argument");
    DAISY_CHECK_ARG(dim_ok(n), "history_csr: n=%lld outside [1, 2^31)", (long long)n);
    DAISY_CHECK_ARG(dim_ok(row_num), "history_csr: row_num=%lld outside [1, 2^31)", (long long)row_num);
    DAISY_CHECK_ARG(dim_ok(col_num), "history_csr: col_num=%lld outside [1, 2^31)", (long long)col_num);
    hipStream_t s = as_stream(stream);
    DeviceArena arena;
    uint64_t *key_a, *key_b;
    int32_t *val_a, *val_b;
    uint32_t *flag, *excl, *start;
    void *temp;
    int64_t *word;           // [0] nnz, [1] the longest row
    const size_t temp_bytes = pair_temp_bytes(n);
    arena.add(&key_a, (size_t)n * sizeof(uint64_t));
    arena.add(&key_b, (size_t)n * sizeof(uint64_t));
    arena.add(&val_a, (size_t)n * sizeof(int32_t));
    arena.add(&val_b, (size_t)n * sizeof(int32_t));
    arena.add(&flag, (size_t)n * sizeof(uint32_t));
    arena.add(&excl, (size_t)n * sizeof(uint32_t));
    arena.add(&start, (size_t)(row_num + 1) * sizeof(uint32_t));
    arena.add(&temp, temp_bytes);
    arena.add(&word, 2 * sizeof(int64_t));
    int rc = arena.alloc("history_csr");
    if (rc != DAISY_OK) return rc;
    ArenaGuard guard{arena};

    const dim3 g = hist_grid(n), gr = hist_grid(row_num + 1), b(kBlock);
    unsigned long long *const longest = reinterpret_cast<unsigned long long *>(word + 1);
    const int col_bits = bits_for(col_num);                 // <= 31, and <= 31 more for the row: the key fits 62 bits
    hipLaunchKernelGGL(k_hist_pair_keys, g, b, 0, s, row, col, n, col_bits, key_a, val_a);
    DAISY_LAUNCH_CHECK();
    // the one sort: (row, col) ascending, equal pairs in frame order
    if ((rc = sort_pairs_u64_i32(temp, temp_bytes, key_a, key_b, val_a, val_b, n, col_bits + bits_for(row_num), s)) != DAISY_OK)
        return rc;
    hipLaunchKernelGGL((k_hist_row_starts<uint64_t, uint32_t>), gr, b, 0, s, key_b, n, row_num, col_bits, start);
    DAISY_LAUNCH_CHECK();
    DAISY_HIP(hipMemsetAsync(word, 0, 2 * sizeof(int64_t), s));
    hipLaunchKernelGGL((k_hist_lens<uint32_t>), hist_grid(row_num), b, 0, s, start, row_num, (int64_t *)nullptr, longest);
    DAISY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_hist_csr_flags, g, b, 0, s, key_b, val_b, val, start, longest, n, col_bits, flag);
    DAISY_LAUNCH_CHECK();
    if ((rc = exclusive_scan_u32(temp, temp_bytes, flag, excl, n, s)) != DAISY_OK) return rc;
    hipLaunchKernelGGL(k_hist_csr_emit, g, b, 0, s, key_b, val_b, flag, excl, val, n, col_bits, out_col, out_val, word);
    DAISY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_hist_row_ptr, gr, b, 0, s, start, flag, excl, n, row_num, row_ptr);
    DAISY_LAUNCH_CHECK();
    DAISY_HIP(hipMemcpyAsync(totals_host, word, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    DAISY_HIP(hipStreamSynchronize(s));     // the arena is released on return
    return DAISY_OK;
}

int daisy_history_first_seen(const int32_t *ids, int64_t n, int64_t id_num, int64_t *out, int64_t *count_host,
                             daisy_stream_t stream) {
    DAISY_CHECK_ARG(ids && out && count_host, "history_first_seen: NULL argument");
    DAISY_CHECK_ARG(dim_ok(n), "history_first_seen: n=%lld outside [1, 2^31)", (long long)n);
    DAISY_CHECK_ARG(dim_ok(id_num), "history_first_seen: id_num=%lld outside [1, 2^31)", (long long)id_num);
    hipStream_t s = as_stream(stream);
    DeviceArena arena;
    int32_t *first;
    uint32_t *flag, *excl;
    void *temp;
    int64_t *word;
    const size_t temp_bytes = exclusive_scan_u32_temp_bytes(n);
    arena.add(&first, (size_t)id_num * sizeof(int32_t));
    arena.add(&flag, (size_t)n * sizeof(uint32_t));
    arena.add(&excl, (size_t)n * sizeof(uint32_t));
    arena.add(&temp, temp_bytes);
    arena.add(&word, sizeof(int64_t));
    int rc = arena.alloc("history_first_seen");
    if (rc != DAISY_OK) return rc;
    ArenaGuard guard{arena};

    const dim3 g = hist_grid(n), b(kBlock);
    hipLaunchKernelGGL(k_hist_fill_i32, hist_grid(id_num), b, 0, s, first, id_num, (int32_t)INT_MAX);
    DAISY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_hist_first_min, g, b, 0, s, ids, n, first);
    DAISY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_hist_head_flags, g, b, 0, s, ids, first, n, flag);
    DAISY_LAUNCH_CHECK();
    if ((rc = exclusive_scan_u32(temp, temp_bytes, flag, excl, n, s)) != DAISY_OK) return rc;
    hipLaunchKernelGGL(k_hist_first_emit, g, b, 0, s, ids, flag, excl, n, out, word);
    DAISY_LAUNCH_CHECK();
    DAISY_HIP(hipMemcpyAsync(count_host, word, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    DAISY_HIP(hipStreamSynchronize(s));     // the arena is released on return
    return DAISY_OK;
}

}  // extern "C"
