// Exact ranks of held-out items over all items: for every requested user and every item of the
// user's target row, the number of eligible items whose sort word (rank_key_f32.h: score descending, a NaN first, equal
// scores by ascending id) is larger than the target's - the position full_rank_users (rank_full.hip) would give it in
// an unbounded list.  No list is built: nothing is appended, compacted or merged.
//   k_frp_slot_*        a request with a target row of L items becomes max(1, ceil(L / 32)) SLOTS of at most kFrpTc
//                       targets each (counts per block of requests, a scan of the blocks, the fill): a long row is just
//                       more slots, so neither pass has a cap on the row length.
//   k_frp_targets       one wave per slot: the 32 target rows of Q on the MFMA's M side, P[u] in column 0 of the N side,
//                       the same v_mfma_f32_32x32x2_f32 chain in ascending k from zero as k_full_rank_tiles, hence its
//                       score bits.  Writes the target's word (all ones: not ranked), its score, and out_pos = 0 or -1.
//   k_frp_count         k_full_rank_tiles' tile loop over 64 slots x a slice of 128-item tiles with another epilogue:
//                       an eligible value is compared with the slot's target words in LDS, the per-target counts are
//                       kept in LDS and added to out_pos once per workgroup with integer atomics.
// Integer sums do not depend on their order: the result is the same for every slice count, schedule and run.
#include "common.h"
#include "mfma.h"
#include "rank_key_f32.h"
#include "rank_tiles_f32.h"                     // the kRt* tile and the helpers shared with k_full_rank_tiles

namespace daisy {

constexpr int kFrpTc = 32;                      // targets of a slot: one MFMA block of pass 1, one LDS row of pass 2
constexpr int kFrpTargetGroups = 1024;          // item slices are added until the grid has about this many workgroups
constexpr uint64_t kFrpNone = ~0ull;            // the word of a target that is not ranked: no word is larger

// LDS of k_frp_count: target words and counts [kFrpTc][64] (slot fastest: the lanes of a wave read neighbouring
// banks), the operand stages, two exclusion masks (tile t uses mask t & 1: the epilogue needs no barrier), and per slot
// the exclusion cursor, row end, user id, first output index and target count
constexpr int kFrpLdsBytes = kFrpTc * kRtBN * (8 + 4) + kRtStageBytes + 2 * kRtMaskBytes + kRtBN * (4 * 8 + 4);

// slots of request b: its target row in blocks of kFrpTc, at least one (the eligible count has to come from somewhere)
__device__ __forceinline__ int64_t frp_slots_of(const int64_t *__restrict__ users, const int64_t *__restrict__ t_indptr,
                                                int64_t b, int64_t n) {
    if (b >= n) return 0;
    const int64_t u = users[b];
    const int64_t len = t_indptr[u + 1] - t_indptr[u];
    return len > kFrpTc ? (len + kFrpTc - 1) / kFrpTc : 1;
}

// exclusive sum over the workgroup's 256 values in a fixed tree; *total: their sum
__device__ __forceinline__ int64_t frp_block_scan(int64_t x, int64_t *s, int64_t *total) {
    const int tid = threadIdx.x;
    s[tid] = x;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {
        const int64_t add = tid >= off ? s[tid - off] : 0;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    const int64_t incl = s[tid];
    *total = s[kBlock - 1];
    __syncthreads();
    return incl - x;
}

__global__ __launch_bounds__(kBlock) void k_frp_slot_counts(const int64_t *__restrict__ users, const int64_t *__restrict__ t_indptr,
                                                            int64_t n, int64_t *__restrict__ bsum) {
    __shared__ int64_t s[kBlock];
    int64_t total;
    frp_block_scan(frp_slots_of(users, t_indptr, (int64_t)blockIdx.x * kBlock + threadIdx.x, n), s, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: bsum becomes its exclusive prefix sum
__global__ __launch_bounds__(kBlock) void k_frp_slot_scan(int64_t *__restrict__ bsum, int64_t n_blocks) {
    __shared__ int64_t s[kBlock];
    int64_t carry = 0;
    for (int64_t base = 0; base < n_blocks; base += kBlock) {
        const int64_t i = base + threadIdx.x;
        int64_t total;
        const int64_t ex = frp_block_scan(i < n_blocks ? bsum[i] : 0, s, &total);
        if (i < n_blocks) bsum[i] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(kBlock) void k_frp_slot_fill(const int64_t *__restrict__ users, const int64_t *__restrict__ t_indptr,
                                                          int64_t n, const int64_t *__restrict__ bsum, int64_t n_slots,
                                                          int64_t *__restrict__ slot_req, int64_t *__restrict__ slot_off) {
    __shared__ int64_t s[kBlock];
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t c = frp_slots_of(users, t_indptr, b, n);
    int64_t total;
    const int64_t first = bsum[blockIdx.x] + frp_block_scan(c, s, &total);
    for (int64_t j = 0; j < c; ++j) {
        if (first + j >= n_slots) break;                    // (never, when t_indptr and n_targets agree)
        slot_req[first + j] = b;
        slot_off[first + j] = j * kFrpTc;
    }
}

// Pass 1.  Lane l feeds A[row l % 32][k l / 32] = Q[target l % 32][k] and B[k l / 32][column l % 32] = P[u][k] in column
// 0, zero elsewhere; lanes 0 and 32 hold column 0 of the result (rows (i / 4) * 8 + (l / 32) * 4 + i % 4).  k runs over
// the same 16-padded range as k_full_rank_tiles.  A target id is range-checked before it indexes Q or i_bias.
__global__ __launch_bounds__(kBlock) void k_frp_targets(
    const float *__restrict__ P, const float *__restrict__ Q, const float *__restrict__ bu, const float *__restrict__ bi,
    const float *__restrict__ b0, int d, int64_t I, const int64_t *__restrict__ users, const int64_t *__restrict__ indptr,
    const int32_t *__restrict__ eitems, const int64_t *__restrict__ t_indptr, const int32_t *__restrict__ t_items,
    const int64_t *__restrict__ out_indptr, int64_t T, const int64_t *__restrict__ slot_req,
    const int64_t *__restrict__ slot_off, int64_t n_slots, uint64_t *__restrict__ words, int32_t *__restrict__ out_pos,
    float *__restrict__ out_scores) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const int64_t slot = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
    if (slot >= n_slots) return;                            // (the same for every lane of the wave)
    const int64_t b = slot_req[slot];
    if (b < 0) return;
    const int64_t u = users[b], off = slot_off[slot];
    const int64_t row_lo = t_indptr[u] + off;
    int64_t len = t_indptr[u + 1] - row_lo;
    len = len > kFrpTc ? kFrpTc : len;
    if (len <= 0) return;                                   // an empty target row: nothing to write
    const int64_t dst0 = out_indptr[b] + off;
    const int r = lane % 32, kh = lane / 32;
    const int64_t tgt = (r < len) ? (int64_t)t_items[row_lo + r] : -1;
    const bool in_range = tgt >= 0 && tgt < I;
    bool excluded = false;
    if (indptr && in_range) {                               // row contents are only compared
        const int64_t hi = indptr[u + 1];
        const int64_t a = rt_lower_bound(eitems, indptr[u], hi, tgt);
        excluded = a < hi && (int64_t)eitems[a] == tgt;
    }
    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const int k_end = (d + kRtBK - 1) / kRtBK * kRtBK;
    for (int k0 = 0; k0 < k_end; k0 += 2) {
        const int k = k0 + kh;
        const bool ka = in_range && k < d, kb = r == 0 && k < d;
        const float qa = Q[ka ? tgt * d + k : 0], pb = P[kb ? u * d + k : 0];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ka ? qa : 0.f, kb ? pb : 0.f, acc, 0, 0, 0);
    }
    float ep_bu = 0.f, ep_b0 = 0.f;
    if (bu) { ep_bu = bu[u]; ep_b0 = b0[0]; }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = rt_acc_item(i, lane);
        const int64_t item = __shfl((long long)tgt, row, kWave);        // every lane takes part in the exchange
        const bool ok = __shfl((int)(in_range && !excluded), row, kWave) != 0;
        if (r != 0 || row >= len || dst0 + row >= T) continue;
        float v = acc[i];
        if (bu && ok) v += (ep_bu + bi[item]) + ep_b0;
        const uint64_t word = fr_word(v, item);
        words[dst0 + row] = ok ? word : kFrpNone;
        out_pos[dst0 + row] = ok ? 0 : -1;
        if (out_scores) out_scores[dst0 + row] = ok ? fr_word_score(word) : -INFINITY;
    }
}

// Pass 2.  The tile loop, the chunk stream and the exclusion walk are k_full_rank_tiles' (rank_full.hip explains them);
// "user" there is "slot" here.  They are a second copy on purpose (rank_tiles_f32.h says what the shared forms cost): a
// change to the loop in one file belongs in the other too.  The one difference is the mask: two buffers here (tile t
// uses t & 1), so this epilogue needs no barrier; one buffer there, so that epilogue must have a workgroup barrier
// after its last mask read (its __syncthreads_or).
template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_frp_count(
    const float *__restrict__ P, const float *__restrict__ Q, const float *__restrict__ bu, const float *__restrict__ bi,
    const float *__restrict__ b0, int d, int64_t I, const int64_t *__restrict__ users, const int64_t *__restrict__ indptr,
    const int32_t *__restrict__ eitems, const int64_t *__restrict__ t_indptr, const int64_t *__restrict__ out_indptr,
    int64_t T, const int64_t *__restrict__ slot_req, const int64_t *__restrict__ slot_off, int64_t n_slots,
    int64_t tiles_per_slice, int64_t n_tiles, const uint64_t *__restrict__ words, int32_t *__restrict__ out_pos,
    int32_t *__restrict__ out_eligible) {
    extern __shared__ __attribute__((aligned(16))) unsigned char frp_lds[];
    uint64_t *tw = reinterpret_cast<uint64_t *>(frp_lds);                       // [kFrpTc][64] target words
    int64_t *cur = reinterpret_cast<int64_t *>(tw + kFrpTc * kRtBN);           // [64] the slice's first exclusion cursor
    int64_t *end = cur + kRtBN;                                                // [64] the exclusion row's end
    int64_t *uid = end + kRtBN;                                                // [64] user id of the slot, -1: empty
    int64_t *dst = uid + kRtBN;                                                // [64] first index into out_pos
    float *As = reinterpret_cast<float *>(dst + kRtBN);                        // [2][kRtBK * kRtLA]
    float *Bs = As + 2 * kRtBK * kRtLA;                                       // [2][kRtBK * kRtLB]
    uint32_t *mask = reinterpret_cast<uint32_t *>(Bs + 2 * kRtBK * kRtLB);    // [2][64][4]: bit = item of the tile
    int *cnt = reinterpret_cast<int *>(mask + 2 * kRtBN * 4);                  // [kFrpTc][64] words above the target
    int *nt = cnt + kFrpTc * kRtBN;                                            // [64] targets of the slot

    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const int wm = wave / 2, wn = wave % 2;
    const int64_t s0 = (int64_t)blockIdx.x * kRtBN;
    const int64_t t_lo = (int64_t)blockIdx.y * tiles_per_slice;
    const int64_t t_hi = (t_lo + tiles_per_slice < n_tiles) ? (t_lo + tiles_per_slice) : n_tiles;

    bool counts_eligible = false;                           // tid < 64: the slot is the first of its request
    if (tid < kRtBN) {
        const int64_t slot = s0 + tid;
        const int64_t b = (slot < n_slots) ? slot_req[slot] : -1;
        int64_t u = -1, lo = 0, hi = 0, d0 = 0;
        int c = 0;
        if (b >= 0) {
            u = users[b];
            const int64_t off = slot_off[slot];
            const int64_t len = t_indptr[u + 1] - t_indptr[u] - off;
            c = (int)(len > kFrpTc ? kFrpTc : (len > 0 ? len : 0));
            d0 = out_indptr[b] + off;
            if (d0 + c > T) c = (int)(T > d0 ? T - d0 : 0);  // (never, when out_indptr is the prefix sum of the rows)
            counts_eligible = off == 0;
            if (indptr) {
                hi = indptr[u + 1];
                lo = rt_lower_bound(eitems, indptr[u], hi, t_lo * kRtBM);   // the slice's first item
            }
        }
        uid[tid] = u;
        cur[tid] = lo;
        end[tid] = hi;
        dst[tid] = d0;
        nt[tid] = c;
    }
    if (__syncthreads_count(tid < kRtBN && uid[tid] >= 0) == 0) return;        // a tile past the last slot
    for (int idx = tid; idx < kFrpTc * kRtBN; idx += kBlock) {
        const int t = idx / kRtBN, sl = idx % kRtBN;
        tw[idx] = (t < nt[sl]) ? words[dst[sl] + t] : kFrpNone;
        cnt[idx] = 0;
    }
    __syncthreads();

    const int64_t my_uid = uid[tid / 4];                    // the slot whose row this thread loads (B operand)
    int64_t wc = cur[tid / 4];
    const int64_t we = end[tid / 4];
    int32_t wv = INT32_MAX;
    const int ul = wn * 32 + lane % 32;                     // the slot whose scores this lane holds
    const int64_t ep_uid = uid[ul];
    const int ep_nt = nt[ul];
    uint64_t ep_min = kFrpNone;                             // the slot's smallest target word: most values lie below it
    for (int t = 0; t < ep_nt; ++t) {
        const uint64_t x = tw[t * kRtBN + ul];
        ep_min = x < ep_min ? x : ep_min;
    }
    float ep_bu = 0.f, ep_b0 = 0.f;
    if (bu && ep_uid >= 0) { ep_bu = bu[ep_uid]; ep_b0 = b0[0]; }
    int elig = 0;                                           // tid < 64: eligible items of slot tid in this slice
    const int kk = (tid % 4) * 4;
    const int n_k = (d + kRtBK - 1) / kRtBK;
    const int64_t total = (t_hi - t_lo) * n_k;
    float ra[kRtAhead][8], rb[kRtAhead][4];
    int64_t li0 = t_lo * kRtBM;
    int lk = 0;
    // no load sits behind a branch: an element outside the tables is read from the table's first element and zeroed
    auto issue = [&](float (&a)[8], float (&b)[4]) {
        const int k = lk + kk;
        auto row_load = [&](const float *__restrict__ Tb, int64_t r, bool row, float *o) {
            if constexpr (VEC) {
                const bool ok = row && k < d;
                const float4 v = *reinterpret_cast<const float4 *>(Tb + (ok ? r * d + k : 0));
                o[0] = ok ? v.x : 0.f; o[1] = ok ? v.y : 0.f; o[2] = ok ? v.z : 0.f; o[3] = ok ? v.w : 0.f;
            } else {
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const bool ok = row && k + x < d;
                    const float v = Tb[ok ? r * d + k + x : 0];
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
    // lane holds slot column (lane % 32) and items (i/4)*8 + (lane/32)*4 + i%4 of each 32x32 block.  No barrier in here:
    // the counts are LDS atomics and the mask of the next tile goes to the other buffer.
    auto epilogue = [&](int64_t i0, const uint32_t *__restrict__ mk) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
            const uint32_t mw = mk[ul * 4 + wm * 2 + mi];
            uint64_t w[16];
            bool any = false;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int bit = rt_acc_item(i, lane);
                const int64_t item = i0 + wm * 64 + mi * 32 + bit;
                float v = acc[mi][i];
                if (bu) v += (ep_bu + bi[item < I ? item : I - 1]) + ep_b0;
                // (fr_word, written out: through the helper this kernel came out 26 VGPRs larger, at one wave per SIMD)
                const uint64_t word = ((uint64_t)fr_key(v) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)item);
                w[i] = (item < I && !((mw >> bit) & 1u)) ? word : 0ull;        // 0: above no target
                any |= w[i] > ep_min;
            }
            if (any) {
                for (int t = 0; t < ep_nt; ++t) {
                    const uint64_t x = tw[t * kRtBN + ul];
                    int c = 0;
#pragma unroll
                    for (int i = 0; i < 16; ++i) c += (w[i] > x) ? 1 : 0;
                    if (c) atomicAdd(&cnt[t * kRtBN + ul], c);
                }
            }
        }
    };
    const int wj = tid % 4;
    auto walk_fetch = [&]() { wv = (wc + wj < we) ? eitems[wc + wj] : INT32_MAX; };
    auto build_mask = [&](int64_t i0, uint32_t *__restrict__ mk) {
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
        mk[tid] = wj == 0 ? m[0] : (wj == 1 ? m[1] : (wj == 2 ? m[2] : m[3]));
        walk_fetch();
    };
    // eligible items of slot tid in the tile at i0: the tile's items below I without the mask's bits
    auto count_eligible = [&](int64_t i0, const uint32_t *__restrict__ mk) {
        if (tid >= kRtBN) return;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t left = I - (i0 + q * 32);         // items of this word that exist
            const uint32_t valid = left >= 32 ? 0xFFFFFFFFu : (left > 0 ? ((1u << left) - 1u) : 0u);
            elig += __popc(valid & ~mk[tid * 4 + q]);
        }
    };

#pragma unroll
    for (int j = 0; j < kRtAhead; ++j) issue(ra[j], rb[j]);
    store(0, ra[0], rb[0]);
    if (indptr) walk_fetch();
    else { mask[tid] = 0u; mask[kBlock + tid] = 0u; }
    __syncthreads();
    int stage = 0, kc = 0, mb = 0;
    int64_t i0 = t_lo * kRtBM;
    for (int64_t g0 = 0; g0 < total; g0 += kRtAhead) {
#pragma unroll
        for (int j = 0; j < kRtAhead; ++j) {
            const int64_t g = g0 + j;
            if (g >= total) break;
            if (kc == 0) {
                if (indptr) build_mask(i0, mask + mb * kBlock);
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[mi][i] = 0.f;
            }
            issue(ra[j], rb[j]);
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
            __syncthreads();                                // (the tile's mask is complete here as well)
            stage ^= 1;
            if (++kc == n_k) {
                kc = 0;
                count_eligible(i0, mask + mb * kBlock);
                epilogue(i0, mask + mb * kBlock);
                i0 += kRtBM;
                mb ^= 1;
            }
        }
    }

    __syncthreads();
    for (int idx = tid; idx < kFrpTc * kRtBN; idx += kBlock) {
        const int t = idx / kRtBN, sl = idx % kRtBN;
        const int c = cnt[idx];
        if (c && t < nt[sl]) atomicAdd(&out_pos[dst[sl] + t], c);       // (a target that is not ranked counted nothing)
    }
    if (out_eligible && tid < kRtBN && counts_eligible && elig) atomicAdd(&out_eligible[slot_req[s0 + tid]], elig);
}

struct FrpLayout {
    int64_t n_slots, n_blocks;
    size_t words, slot_req, slot_off, bsum, total;
};
static FrpLayout frp_layout(int64_t n, int64_t n_targets) {
    FrpLayout l;
    l.n_slots = n + n_targets / kFrpTc;                     // sum over requests of max(1, ceil(len / Tc)) is at most this
    l.n_blocks = (n + kBlock - 1) / kBlock;
    l.words = 0;
    l.slot_req = align_up((size_t)(n_targets > 0 ? n_targets : 1) * 8);
    l.slot_off = l.slot_req + align_up((size_t)l.n_slots * 8);
    l.bsum = l.slot_off + align_up((size_t)l.n_slots * 8);
    l.total = l.bsum + align_up((size_t)l.n_blocks * 8);
    return l;
}
static bool frp_sizes_ok(int64_t n, int64_t n_targets) {
    return n > 0 && n <= ((int64_t)1 << 31) && n_targets >= 0 && n_targets <= ((int64_t)1 << 40);
}

}  // namespace daisy

using namespace daisy;

extern "C" {

size_t daisy_full_rank_positions_workspace_bytes(int64_t n, int64_t n_targets) {
    if (!frp_sizes_ok(n, n_targets)) return 0;
    return frp_layout(n, n_targets).total;
}

int daisy_full_rank_positions(const float *P, const float *Q, const float *u_bias, const float *i_bias, const float *bias,
                              int32_t d, int64_t item_num, const int64_t *users, int64_t n, const int64_t *excl_indptr,
                              const int32_t *excl_items, const int64_t *t_indptr, const int32_t *t_items,
                              const int64_t *out_indptr, int64_t n_targets, int32_t item_slices, int32_t *out_pos,
                              float *out_scores, int32_t *out_eligible, void *workspace, size_t workspace_bytes,
                              daisy_stream_t stream) {
    DAISY_CHECK_ARG(P && Q && users && t_indptr && t_items && out_indptr && out_pos && workspace,
                    "full_rank_positions: NULL argument");
    DAISY_CHECK_ARG((u_bias && i_bias && bias) || (!u_bias && !i_bias && !bias),
                    "full_rank_positions: u_bias, i_bias and bias are given together or not at all");
    DAISY_CHECK_ARG((excl_indptr != nullptr) == (excl_items != nullptr),
                    "full_rank_positions: excl_indptr and excl_items are given together or not at all");
    DAISY_CHECK_ARG(n > 0 && n <= ((int64_t)1 << 31), "full_rank_positions: bad request count n=%lld", (long long)n);
    DAISY_CHECK_ARG(n_targets >= 0 && n_targets <= ((int64_t)1 << 40), "full_rank_positions: bad target count n_targets=%lld",
                    (long long)n_targets);
    DAISY_CHECK_ARG(item_num > 0 && item_num < ((int64_t)1 << 31), "full_rank_positions: item_num=%lld outside [1, 2^31)",
                    (long long)item_num);
    DAISY_CHECK_ARG(d >= 1 && d <= kMaxD, "full_rank_positions: unsupported factor count d=%d (1..%d)", d, kMaxD);
    DAISY_CHECK_ARG(item_slices >= 0, "full_rank_positions: item_slices=%d is negative", item_slices);
    DAISY_CHECK_ARG(workspace_bytes >= daisy_full_rank_positions_workspace_bytes(n, n_targets),
                    "full_rank_positions: workspace too small");
    const FrpLayout lay = frp_layout(n, n_targets);
    char *ws = static_cast<char *>(workspace);
    uint64_t *words = reinterpret_cast<uint64_t *>(ws + lay.words);
    int64_t *slot_req = reinterpret_cast<int64_t *>(ws + lay.slot_req);
    int64_t *slot_off = reinterpret_cast<int64_t *>(ws + lay.slot_off);
    int64_t *bsum = reinterpret_cast<int64_t *>(ws + lay.bsum);
    int64_t per, n_tiles;
    int S;
    rt_slices(lay.n_slots, item_num, item_slices, kFrpTargetGroups, &per, &n_tiles, &S);
    hipStream_t s = as_stream(stream);
    auto kern = rt_vec(d, P, Q) ? k_frp_count<true> : k_frp_count<false>;
    DAISY_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kFrpLdsBytes));

    DAISY_HIP(hipMemsetAsync(slot_req, 0xFF, (size_t)lay.n_slots * 8, s));      // -1: a slot no request fills
    if (out_eligible) DAISY_HIP(hipMemsetAsync(out_eligible, 0, (size_t)n * sizeof(int32_t), s));
    const dim3 blocks((unsigned)lay.n_blocks), block(kBlock);
    hipLaunchKernelGGL(k_frp_slot_counts, blocks, block, 0, s, users, t_indptr, n, bsum);
    DAISY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_frp_slot_scan, dim3(1), block, 0, s, bsum, lay.n_blocks);
    DAISY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_frp_slot_fill, blocks, block, 0, s, users, t_indptr, n, bsum, lay.n_slots, slot_req, slot_off);
    DAISY_LAUNCH_CHECK();
    if (n_targets > 0) {
        const int64_t G1 = (lay.n_slots + kBlock / kWave - 1) / (kBlock / kWave);
        hipLaunchKernelGGL(k_frp_targets, dim3((unsigned)G1), block, 0, s, P, Q, u_bias, i_bias, bias, (int)d, item_num, users,
                           excl_indptr, excl_items, t_indptr, t_items, out_indptr, n_targets, slot_req, slot_off, lay.n_slots,
                           words, out_pos, out_scores);
        DAISY_LAUNCH_CHECK();
    }
    const int64_t UT = (lay.n_slots + kRtBN - 1) / kRtBN;
    hipLaunchKernelGGL(kern, dim3((unsigned)UT, (unsigned)S), block, kFrpLdsBytes, s, P, Q, u_bias, i_bias, bias, (int)d,
                       item_num, users, excl_indptr, excl_items, t_indptr, out_indptr, n_targets, slot_req, slot_off,
                       lay.n_slots, per, n_tiles, words, out_pos, out_eligible);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

}  // extern "C"
