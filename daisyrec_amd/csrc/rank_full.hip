// Full ranking of many users in two launches: score every user against every item, drop the
// items of the user's exclusion row, keep the topk best - without ever materialising a [users, items] score tile.
//   k_full_rank_tiles   a workgroup owns 64 users and a contiguous slice of whole 128-item tiles.  Scores come from the
//                       fp32 MFMA (32x32x2, items on the M side, users on the N side: a lane holds 16 items of ONE user),
//                       LDS-staged like gemm_f32_tile, with four k chunks in flight in registers.  The epilogue turns each value
//                       into a 64-bit sort word (order-preserving score key | 0xFFFFFFFF - item), tests it against the
//                       tile's exclusion mask and the user's k-th-best threshold and appends it to the user's candidate
//                       buffer in LDS; a buffer that could overflow in the next step is compacted to its topk largest
//                       words by one wave (bitonic sort in registers) and the threshold rises.
//   k_full_rank_merge   per user: the topk largest of the slices' partial lists, decoded to ids (and scores).
// The order on sort words is total (score descending, item ascending), so the top-k SET is unique and the result does
// not depend on append order, wave scheduling or the slice count.
#include "common.h"
#include "mfma.h"
#include "rank_key_f32.h"                       // fr_word: the sort word and its halves
#include "rank_tiles_f32.h"                     // the kRt* tile and the helpers shared with k_frp_count

namespace daisy {

constexpr int kFrTopkCap = 128;                 // the contract's cap: candidate buffers of 64 users live in LDS
constexpr int kFrSort = 256;                    // words one wave sorts: 4 per lane
constexpr int kFrBuf = 224;                     // candidate words per user
constexpr int kFrStep = 64;                     // most words ONE epilogue step appends to one user: 2 waves x 32 items
constexpr int kFrLimit = kFrBuf - kFrStep;      // a buffer holding more than this is compacted before the next step
static_assert(kFrLimit >= kFrTopkCap && kFrBuf <= kFrSort, "a compacted buffer must leave room for one step");

// candidate buffers, the operand stages and ONE exclusion mask (the epilogue's barrier frees it for the next tile), and
// per user the threshold, exclusion cursor, row end, user id and count
constexpr int kFrLdsBytes = kRtBN * kFrBuf * 8 + kRtStageBytes + kRtMaskBytes + kRtBN * (8 * 4 + 4);
// item slices are added until the grid has about this many workgroups (one workgroup per CU is resident: its candidate
// buffers take most of the LDS)
constexpr int kFrTargetGroups = 512;

// 256 words of a wave, element e = lane * 4 + r in w[r], into descending order: a bitonic network whose strides below
// 4 stay inside the lane and whose wider ones are one lane exchange per word.  No LDS, no barrier.
__device__ __forceinline__ void fr_sort_desc(uint64_t (&w)[4], int lane) {
#pragma unroll
    for (int k = 2; k <= kFrSort; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j >= 1; j >>= 1) {
            if (j >= 4) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int e = lane * 4 + r;
                    const uint64_t o = rt_shfl_xor(w[r], j >> 2);
                    const bool keep_max = ((e & j) == 0) == ((e & k) == 0);
                    const uint64_t hi = (w[r] > o) ? w[r] : o, lo = (w[r] > o) ? o : w[r];
                    w[r] = keep_max ? hi : lo;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (r & j) continue;
                    const int e = lane * 4 + r;
                    const bool desc = (e & k) == 0;
                    const uint64_t a = w[r], b = w[r | j];
                    const uint64_t hi = (a > b) ? a : b, lo = (a > b) ? b : a;
                    w[r] = desc ? hi : lo;
                    w[r | j] = desc ? lo : hi;
                }
            }
        }
    }
}

// One wave: the candidate words of user slot `u` (count c <= kFrBuf) sorted; the topk largest go back to the head of
// the buffer (or, dst != nullptr, to dst[0 .. topk), zero-filled) and the threshold becomes the topk-th of them.
__device__ __forceinline__ void fr_compact(uint64_t *__restrict__ ubuf, int c, int topk, int lane, int *cnt_u,
                                           uint64_t *thr_u, uint64_t *__restrict__ dst) {
    uint64_t w[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int e = lane * 4 + r;
        w[r] = (e < c) ? ubuf[e] : 0ull;
    }
    fr_sort_desc(w, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int e = lane * 4 + r;
        if (e < topk) {
            if (dst) dst[e] = w[r];
            else ubuf[e] = w[r];
        }
        if (!dst && e == topk - 1) *thr_u = (c >= topk) ? w[r] : 0ull;
    }
    if (!dst && lane == 0) *cnt_u = (c < topk) ? c : topk;
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_full_rank_tiles(
    const float *__restrict__ P, const float *__restrict__ Q, const float *__restrict__ bu, const float *__restrict__ bi,
    const float *__restrict__ b0, int d, int64_t I, const int64_t *__restrict__ users, int64_t n,
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ eitems, int topk, int64_t tiles_per_slice,
    int64_t n_tiles, int S, uint64_t *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fr_lds[];
    uint64_t *buf = reinterpret_cast<uint64_t *>(fr_lds);                       // [64][kFrBuf]
    float *As = reinterpret_cast<float *>(buf + kRtBN * kFrBuf);                // [2][kRtBK * kRtLA]
    float *Bs = As + 2 * kRtBK * kRtLA;                                         // [2][kRtBK * kRtLB]
    uint32_t *mask = reinterpret_cast<uint32_t *>(Bs + 2 * kRtBK * kRtLB);      // [64][4]: bit = item of the tile
    uint64_t *thr = reinterpret_cast<uint64_t *>(mask + kRtBN * 4);             // [64] k-th best word so far (0: none)
    int64_t *cur = reinterpret_cast<int64_t *>(thr + kRtBN);                    // [64] the slice's first cursor into the exclusion
    int64_t *end = cur + kRtBN;                                                 // [64] row and the row's end (read once, below)
    int64_t *uid = end + kRtBN;                                                 // [64] user id of the slot, -1: past n
    int *cnt = reinterpret_cast<int *>(uid + kRtBN);                            // [64] words in the buffer

    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const int wm = wave / 2, wn = wave % 2;
    const int64_t u0 = (int64_t)blockIdx.x * kRtBN;
    const int s = blockIdx.y;
    const int64_t t_lo = (int64_t)s * tiles_per_slice;
    const int64_t t_hi = (t_lo + tiles_per_slice < n_tiles) ? (t_lo + tiles_per_slice) : n_tiles;

    if (tid < kRtBN) {
        const int64_t slot = u0 + tid;
        const int64_t u = (slot < n) ? users[slot] : -1;
        uid[tid] = u;
        cnt[tid] = 0;
        thr[tid] = 0ull;
        int64_t lo = 0, hi = 0;
        if (indptr && u >= 0) {
            hi = indptr[u + 1];
            lo = rt_lower_bound(eitems, indptr[u], hi, t_lo * kRtBM);       // the slice's first item
        }
        cur[tid] = lo;
        end[tid] = hi;
    }
    __syncthreads();

    const int64_t my_uid = uid[tid / 4];                    // the user whose row this thread loads (B operand)
    int64_t wc = cur[tid / 4];                              // exclusion walk of that user: cursor, row end, and
    const int64_t we = end[tid / 4];                        // the entry this thread looks at next
    int32_t wv = INT32_MAX;
    const int ul = wn * 32 + lane % 32;                     // the user slot whose scores this lane holds
    const int64_t ep_uid = uid[ul];
    float ep_bu = 0.f, ep_b0 = 0.f;
    if (bu && ep_uid >= 0) { ep_bu = bu[ep_uid]; ep_b0 = b0[0]; }
    const int kk = (tid % 4) * 4;
    const int n_k = (d + kRtBK - 1) / kRtBK;
    // The workgroup's work is ONE stream of chunks, (item tile, k chunk) with the tile outermost.  Chunk g sits in LDS
    // stage g & 1; chunks g + 1 .. g + kRtAhead are in flight from memory into a ring of registers (slot = chunk %
    // kRtAhead), so a load has three chunks of MFMAs - and, across a tile boundary, the epilogue - to arrive in: the
    // candidate buffers leave room for ONE workgroup per CU, so no other wave hides a wait for memory.
    const int64_t total = (t_hi - t_lo) * n_k;
    float ra[kRtAhead][8], rb[kRtAhead][4];
    int64_t li0 = t_lo * kRtBM;                             // the next chunk to load: its tile's first item, its k
    int lk = 0;
    // No load sits behind a branch: an element outside the tables is read from the table's first element and zeroed
    // afterwards (Row::load_clamped's flavour), and chunks past the stream's end are issued like the others (their
    // rows clamp the same way).  Loads return in order, so a wait for a chunk is a count of the loads issued after it;
    // a load behind control flow makes the compiler drain them all (with guarded loads every wait came out as vmcnt(0)).
    auto issue = [&](float (&a)[8], float (&b)[4]) {
        const int k = lk + kk;
        auto row_load = [&](const float *__restrict__ T, int64_t r, bool row, float *o) {
            if constexpr (VEC) {                            // d % 4 == 0: k < d covers k .. k + 3
                const bool ok = row && k < d;
                const float4 v = *reinterpret_cast<const float4 *>(T + (ok ? r * d + k : 0));
                o[0] = ok ? v.x : 0.f; o[1] = ok ? v.y : 0.f; o[2] = ok ? v.z : 0.f; o[3] = ok ? v.w : 0.f;
            } else {
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const bool ok = row && k + x < d;
                    const float v = T[ok ? r * d + k + x : 0];
                    o[x] = ok ? v : 0.f;
                }
            }
        };
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int64_t item = li0 + tid / 4 + q * 64;
            row_load(Q, item, item < I, a + 4 * q);
        }
        row_load(P, my_uid, my_uid >= 0, b);
        lk += kRtBK;
        if (lk >= d) { lk = 0; li0 += kRtBM; }
    };
    auto store = [&](int stage, const float (&a)[8], const float (&b)[4]) {
        float *A = As + stage * kRtBK * kRtLA, *B = Bs + stage * kRtBK * kRtLB;
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int x = 0; x < 4; ++x) A[(kk + x) * kRtLA + tid / 4 + q * 64] = a[4 * q + x];
#pragma unroll
        for (int x = 0; x < 4; ++x) B[(kk + x) * kRtLB + tid / 4] = b[x];
    };

    floatx16 acc[2];
    // lane holds user column (lane % 32) and items rt_acc_item(i, lane) of each 32x32 block: the C/D map gemm_epilogue
    // decodes.  One step per mi: at most kFrStep words per user, then the full buffers are compacted.  There is ONE
    // mask buffer, which the next tile's build_mask overwrites: the __syncthreads_or below is the workgroup barrier that
    // must follow the last mask read (k_frp_count, the second copy of this stream, has two buffers and no barrier).
    auto epilogue = [&](int64_t i0) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
            const uint64_t th = thr[ul];
            const uint32_t mw = mask[ul * 4 + wm * 2 + mi];
            int full = 0;
            if (ep_uid >= 0) {
                // branch-free over the 16 values, then ONE claim of buffer places per lane: an LDS atomic per passing
                // value cost a round trip each (8 of 30 ms at n = 138 k, topk = 50)
                uint64_t w[16];
                uint32_t pm = 0u;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int bit = rt_acc_item(i, lane);
                    const int64_t item = i0 + wm * 64 + mi * 32 + bit;
                    float v = acc[mi][i];
                    if (bu) v += (ep_bu + bi[item < I ? item : I - 1]) + ep_b0;
                    w[i] = fr_word(v, item);
                    const bool pass = item < I && !((mw >> bit) & 1u) && w[i] > th;
                    pm |= pass ? (1u << i) : 0u;
                }
                if (pm) {
                    const int np = __popc(pm);
                    int pos = atomicAdd(&cnt[ul], np);
                    full = pos + np > kFrLimit;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        if (pm & (1u << i)) {
                            if (pos < kFrBuf) buf[ul * kFrBuf + pos] = w[i];    // (always: cnt <= kFrLimit before the step)
                            ++pos;
                        }
                    }
                }
            }
            if (__syncthreads_or(full)) {                   // some buffer could overflow in the next step
                for (int u = wave; u < kRtBN; u += kBlock / kWave) {
                    const int c = cnt[u];
                    if (c > kFrLimit)
                        fr_compact(buf + u * kFrBuf, c < kFrBuf ? c : kFrBuf, topk, lane, cnt + u, thr + u, nullptr);
                }
                __syncthreads();
            }
        }
    };
    // the tile's exclusion bits: four threads walk a user's row from its cursor, entry p by the thread p % 4 == its
    // place in the quad; the cursor (the first entry at or past the tile's end) only moves forward
    // The cursor lives in the quad's registers, and the entry a thread will look at first was loaded a tile ago (wv:
    // entry wc + wj, or the sentinel past the row's end): in the common case - no entry of the row inside this tile -
    // the walk waits for no load, so it does not drain the chunks in flight either.
    const int wj = tid % 4;
    auto walk_fetch = [&]() { wv = (wc + wj < we) ? eitems[wc + wj] : INT32_MAX; };
    auto build_mask = [&](int64_t i0) {
        uint32_t m[4] = {0u, 0u, 0u, 0u};
        int64_t p = wc + wj;
        int64_t it = (int64_t)wv;
        while (p < we && it < i0 + kRtBM) {
            if (it >= i0) {
                const int b = (int)(it - i0);
#pragma unroll
                for (int q = 0; q < 4; ++q) m[q] |= (b >> 5) == q ? (1u << (b & 31)) : 0u;
            }
            p += 4;
            it = (p < we) ? (int64_t)eitems[p] : (int64_t)INT32_MAX;
        }
        uint64_t pm = (uint64_t)(p < we ? p : we);
#pragma unroll
        for (int x = 1; x <= 2; x <<= 1) {
            const uint64_t o = rt_shfl_xor(pm, x);
            pm = o < pm ? o : pm;
#pragma unroll
            for (int q = 0; q < 4; ++q) m[q] |= (uint32_t)__shfl_xor((int)m[q], x, kWave);
        }
        wc = (int64_t)pm;
        mask[tid] = wj == 0 ? m[0] : (wj == 1 ? m[1] : (wj == 2 ? m[2] : m[3]));
        walk_fetch();
    };

#pragma unroll
    for (int j = 0; j < kRtAhead; ++j) issue(ra[j], rb[j]);
    store(0, ra[0], rb[0]);
    if (indptr) walk_fetch();
    else mask[tid] = 0u;
    __syncthreads();
    int stage = 0, kc = 0;
    int64_t i0 = t_lo * kRtBM;
    for (int64_t g0 = 0; g0 < total; g0 += kRtAhead) {
#pragma unroll
        for (int j = 0; j < kRtAhead; ++j) {
            const int64_t g = g0 + j;
            if (g >= total) break;
            if (kc == 0) {
                if (indptr) build_mask(i0);
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[mi][i] = 0.f;
            }
            issue(ra[j], rb[j]);                    // chunk g + kRtAhead into chunk g's slot: g went to LDS an iteration ago
            const float *as = As + stage * kRtBK * kRtLA + (lane / 32) * kRtLA + wm * 64 + lane % 32;
            const float *bs = Bs + stage * kRtBK * kRtLB + (lane / 32) * kRtLB + wn * 32 + lane % 32;
            float a[2][2], b[2];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) a[0][mi] = as[mi * 32];
            b[0] = bs[0];
#pragma unroll
            for (int ks = 0; ks < kRtBK / 2; ++ks) {
                const int c = ks & 1, nx = c ^ 1;
                if (ks + 1 < kRtBK / 2) {
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi) a[nx][mi] = as[(2 * ks + 2) * kRtLA + mi * 32];
                    b[nx] = bs[(2 * ks + 2) * kRtLB];
                }
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
                    acc[mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c][mi], b[c], acc[mi], 0, 0, 0);
            }
            if (g + 1 < total) store(stage ^ 1, ra[(j + 1) % kRtAhead], rb[(j + 1) % kRtAhead]);
            __syncthreads();
            stage ^= 1;
            if (++kc == n_k) {
                kc = 0;
                epilogue(i0);
                i0 += kRtBM;
            }
        }
    }

    for (int u = wave; u < kRtBN; u += kBlock / kWave) {
        if (uid[u] < 0) continue;
        const int c = cnt[u];
        fr_compact(buf + u * kFrBuf, c < kFrBuf ? c : kFrBuf, topk, lane, nullptr, nullptr,
                   part + ((u0 + u) * S + s) * topk);
    }
}

// one wave per user: the topk largest of the S * topk partial words (zero: an empty position), 128 new words per round
// beside the best 128 so far
__global__ __launch_bounds__(kBlock) void k_full_rank_merge(const uint64_t *__restrict__ part, int64_t n, int S, int topk,
                                                            int64_t *__restrict__ ids, float *__restrict__ scores) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int64_t u = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
    if (u >= n) return;
    const int64_t total = (int64_t)S * topk;
    const uint64_t *__restrict__ src = part + u * total;
    uint64_t w[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int e = lane * 4 + r;
        w[r] = (e < total) ? src[e] : 0ull;
    }
    fr_sort_desc(w, lane);
    for (int64_t base = kFrSort; base < total; base += kFrSort / 2) {
        if (lane >= kWave / 2) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t e = base + (lane - kWave / 2) * 4 + r;
                w[r] = (e < total) ? src[e] : 0ull;
            }
        }
        fr_sort_desc(w, lane);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int e = lane * 4 + r;
        if (e >= topk) continue;
        const bool none = w[r] == 0ull;
        ids[u * topk + e] = none ? (int64_t)-1 : fr_word_item(w[r]);
        if (scores) scores[u * topk + e] = none ? -INFINITY : fr_word_score(w[r]);
    }
}

}  // namespace daisy

using namespace daisy;

extern "C" {

size_t daisy_full_rank_users_workspace_bytes(int64_t n, int64_t item_num, int32_t topk, int32_t item_slices) {
    if (n <= 0 || item_num <= 0 || item_num >= ((int64_t)1 << 31) || topk <= 0 || topk > kFrTopkCap || item_slices < 0 ||
        n > ((int64_t)1 << 36))
        return 0;
    int64_t per, T;
    int S;
    rt_slices(n, item_num, item_slices, kFrTargetGroups, &per, &T, &S);
    return align_up((size_t)n * (size_t)S * (size_t)topk * 8);
}

int daisy_full_rank_users(const float *P, const float *Q, const float *u_bias, const float *i_bias, const float *bias,
                          int32_t d, int64_t item_num, const int64_t *users, int64_t n, const int64_t *excl_indptr,
                          const int32_t *excl_items, int32_t topk, int32_t item_slices, int64_t *out_ids,
                          float *out_scores, void *workspace, size_t workspace_bytes, daisy_stream_t stream) {
    DAISY_CHECK_ARG(P && Q && users && out_ids && workspace, "full_rank_users: NULL argument");
    DAISY_CHECK_ARG((u_bias && i_bias && bias) || (!u_bias && !i_bias && !bias),
                    "full_rank_users: u_bias, i_bias and bias are given together or not at all");
    DAISY_CHECK_ARG((excl_indptr != nullptr) == (excl_items != nullptr),
                    "full_rank_users: excl_indptr and excl_items are given together or not at all");
    DAISY_CHECK_ARG(n > 0 && n <= ((int64_t)1 << 36), "full_rank_users: bad user count n=%lld", (long long)n);
    DAISY_CHECK_ARG(item_num > 0 && item_num < ((int64_t)1 << 31), "full_rank_users: item_num=%lld outside [1, 2^31)",
                    (long long)item_num);
    DAISY_CHECK_ARG(topk <= kFrTopkCap, "full_rank_users: topk=%d above the cap of %d (the candidate buffers live in LDS)",
                    topk, kFrTopkCap);
    DAISY_CHECK_ARG(topk >= 1 && topk <= item_num, "full_rank_users: topk=%d outside [1, item_num=%lld]", topk,
                    (long long)item_num);
    DAISY_CHECK_ARG(d >= 1 && d <= kMaxD, "full_rank_users: unsupported factor count d=%d (1..%d)", d, kMaxD);
    DAISY_CHECK_ARG(item_slices >= 0, "full_rank_users: item_slices=%d is negative", item_slices);
    DAISY_CHECK_ARG(workspace_bytes >= daisy_full_rank_users_workspace_bytes(n, item_num, topk, item_slices),
                    "full_rank_users: workspace too small");
    int64_t per, T;
    int S;
    rt_slices(n, item_num, item_slices, kFrTargetGroups, &per, &T, &S);
    hipStream_t s = as_stream(stream);
    auto kern = rt_vec(d, P, Q) ? k_full_rank_tiles<true> : k_full_rank_tiles<false>;      // float4 rows, or element by element
    DAISY_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kFrLdsBytes));
    uint64_t *part = static_cast<uint64_t *>(workspace);
    const int64_t UT = (n + kRtBN - 1) / kRtBN;
    hipLaunchKernelGGL(kern, dim3((unsigned)UT, (unsigned)S), dim3(kBlock), kFrLdsBytes, s, P, Q, u_bias, i_bias,
                       bias, (int)d, item_num, users, n, excl_indptr, excl_items, (int)topk, per, T, S, part);
    DAISY_LAUNCH_CHECK();
    const int64_t MG = (n + kBlock / kWave - 1) / (kBlock / kWave);
    hipLaunchKernelGGL(k_full_rank_merge, dim3((unsigned)MG), dim3(kBlock), 0, s, part, n, S, (int)topk, out_ids, out_scores);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // extern "C"
