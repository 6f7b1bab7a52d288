// NeuMF's embedding gradients (the last step of daisy_neumf_step_grads, csrc/neumf.hip): g.{uG,iG,uM,iM} += the rows'
// gradients and the regulariser gradients exactly as NeuMFRecommender.py:149-167 lists them, without atomics - every table
// row has one owner that adds its rows' contributions in ascending row order, so two runs give the same bits.
//   small steps (<= kScanMaxRows rows, fp32)   k_nmf_scatter_scan (or k_nmf_scatter_small), one launch
//   otherwise, the owner chain                 rows grouped by table row (the counting pass k_cs_*, or two radix sorts), then
//                                              per table a segmented sum over the grouped list (segsum_rows, segsum.hip:
//                                              k_item_grad_chunked) and k_nmf_table_commit*: the regulariser terms are
//                                              count * f(row) per table row (integer counts)
// (With ml-1m's 6040 users a batch of 524 288 rows hits every user row ~87 times: fp32 atomics serialise on those addresses.)
#include <stdlib.h>

#include "common.h"
#include "neumf_internal.h"
#include "segsum.h"

namespace daisy {

// ---------------------------------------------------------------------------------------------
// Round 6: the embedding gradients of a SMALL step (at most 1024 rows: the reference's own batch of 256 samples is 512) in
// one launch - sixteen workgroups per side - instead of the ~22 launches of the owner-based scatter below (keys, two sorts, entry
// lists, four segmented reductions with their edge launches, four commits): at that size every one of them is a few
// microseconds of launch latency around almost no work, and together they were a third of the 300 us step.
// Per side: the rows' (table row, row) pairs are sorted in LDS (bitonic, one element per thread); a lane group owns each
// table row that occurs and adds its rows' contributions in ascending row order (deterministic), then the regulariser terms
// of NeuMFRecommender.py:149-167 from the run's own counts, and writes the four gradient rows.
// ---------------------------------------------------------------------------------------------
constexpr int kScatterSmallRows = 1024;       // threads of the small-step scatter kernels (and the most rows the sorting one takes)
// the scanning kernel's workgroup: 16 step rows (one 16-lane group each, four waves) up to 2048 rows, 32 beyond - every workgroup
// holds ALL keys of the step in LDS and compares its rows with them, a wave scanning for its four rows at once: the scan's
// length does not depend on the workgroup's size, so the smallest one that still gives one workgroup per CU spreads it best
static int scan_block(int64_t R) { return R <= 2048 ? 256 : 512; }      // (64 groups x 128 rounds of masks would not fit beside 8192 keys)
__global__ __launch_bounds__(kScatterSmallRows) void k_nmf_scatter_small(daisy_neumf_params p, daisy_neumf_params g, PairSrc src,
                                                                        int R, int d, int dm, int model, int pointwise,
                                                                        const float *__restrict__ dpred,
                                                                        const float *__restrict__ DX0,
                                                                        const double *__restrict__ stats, float reg_1,
                                                                        float reg_2) {
    __shared__ uint32_t comp[kScatterSmallRows];          // table row << 10 | step row; padding sorts last
    // (16 workgroups per side: every one sorts the whole list - microseconds - and owns the runs whose heads fall on its
    // share of the positions; two workgroups walked ~250 runs each through dependent loads: 90 us)
    const int side = blockIdx.x, tid = threadIdx.x;
    {
        uint32_t c = 0xFFFFFFFFu;
        if (tid < R) {
            int64_t user, item;
            pair_ids(src, tid, user, item);
            c = ((uint32_t)(side ? item : user) << 10) | (uint32_t)tid;
        }
        comp[tid] = c;
    }
    __syncthreads();
    for (int k = 2; k <= kScatterSmallRows; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int other = tid ^ j;
            if (other > tid) {
                const uint32_t a = comp[tid], b = comp[other];
                const bool up = (tid & k) == 0;
                if ((a > b) == up) { comp[tid] = b; comp[other] = a; }
            }
            __syncthreads();
        }
    auto inv = [&](int k) { const double n = stats[DAISY_NST_NORM + k]; return (n > 0.0) ? (float)((double)reg_2 / n) : 0.f; };
    const float i_m = inv(side ? 3 : 1), i_g = inv(side ? 2 : 0), i_neg = 2.f * inv(4);
    const int lane = tid % 16, group = tid / 16;
    const float *tabM = side ? p.iM : p.uM, *tabG = side ? p.iG : p.uG, *otherG = side ? p.uG : p.iG;
    float *gM = side ? g.iM : g.uM, *gG = side ? g.iG : g.uG;
    for (int e = (int)blockIdx.y * (kScatterSmallRows / 16) + group; e < R; e += (int)gridDim.y * (kScatterSmallRows / 16)) {
        const uint32_t row = comp[e] >> 10;
        if (e > 0 && (comp[e - 1] >> 10) == row) continue;            // the head of a run owns the table row
        int run = 1;
        while (e + run < R && (comp[e + run] >> 10) == row) ++run;
        float npos = 0.f, nneg = 0.f;
        for (int q = 0; q < run; ++q) { if ((int64_t)(comp[e + q] & 1023u) < src.B) npos += 1.f; else nneg += 1.f; }
        // MLP table: the rows' input gradients (this side's half of dX0), the regulariser on the positive rows' occurrences
        for (int c = lane; c < dm; c += 16) {
            float v = 0.f;
            if (model != DAISY_NEUMF_GMF)
                for (int q = 0; q < run; ++q) v += DX0[(int64_t)(comp[e + q] & 1023u) * (2 * dm) + side * dm + c];
            if (npos > 0.f) { const float w = tabM[(int64_t)row * dm + c]; v += fmaf(npos * i_m, w, reg_1 * npos * sgn(w)); }
            if (v != 0.f) gM[(int64_t)row * dm + c] += v;
        }
        // GMF table: Wp[c] x sum of dpred[r] x the OTHER table's row; the negative item's rows count twice in the regulariser
        for (int c = lane; c < d; c += 16) {
            float v = 0.f;
            if (model != DAISY_NEUMF_MLP) {
                for (int q = 0; q < run; ++q) {
                    const int64_t r = comp[e + q] & 1023u;
                    int64_t user, item;
                    pair_ids(src, r, user, item);
                    v = fmaf(dpred[r], otherG[(side ? user : item) * d + c], v);
                }
                v *= p.Wp[c];
            }
            const float na = npos, nb = (side && !pointwise) ? nneg : 0.f;
            if (na + nb > 0.f) {
                const float w = tabG[(int64_t)row * d + c];
                v += fmaf(na * i_g + nb * i_neg, w, reg_1 * (na + 2.f * nb) * sgn(w));
            }
            if (v != 0.f) gG[(int64_t)row * d + c] += v;
        }
    }
}

// The same without the sort, and for steps of up to kScanMaxRows rows: a workgroup per 16 (32) step rows, a 16-lane group per
// row.  Every workgroup holds the step's keys in LDS; a wave compares them, 64 per round, with the keys of its four rows - a
// ballot is the round's mask of rows with the same user (item) - and keeps the rounds with a match; a row whose key occurred
// earlier in the step leaves (the first occurrence owns the table row), an owner walks its masks - the matching rows in
// ascending order, the order of the sorted list - with all of a matched row's columns in flight at once.  Same sums in the
// same order as k_nmf_scatter_small: bit-identical gradients (tests/test_gpu_neumf.py).  The scan is O(rows^2 / 64) per side:
// 3 us at 512 rows, 11 at 4096, 17 at 8192 (profiles/r06_neumf_small_steps.txt) - beyond that the counting pass below.
template <int NT>
__global__ __launch_bounds__(kScatterSmallRows) void k_nmf_scatter_scan(daisy_neumf_params p, daisy_neumf_params g, PairSrc src,
                                                                       int R, int d, int dm, int model, int pointwise,
                                                                       const float *__restrict__ dpred,
                                                                       const float *__restrict__ DX0,
                                                                       const double *__restrict__ stats, float reg_1,
                                                                       float reg_2) {
    extern __shared__ __attribute__((aligned(16))) unsigned char scan_lds[];
#ifdef DAISY_SCAN_PROF
    long long sprof[6] = {0, 0, 0, 0, 0, 0}, spt0 = wall_clock64();
#define SCAN_MARK(k) { const long long now_ = wall_clock64(); sprof[k] += now_ - spt0; spt0 = now_; }
#else
#define SCAN_MARK(k)
#endif
    const int side = blockIdx.x, tid = threadIdx.x;
    const int rounds = (R + 63) / 64;
    const int gpb = (int)blockDim.x / 16;              // 16-lane groups (= step rows) of this workgroup: 16, 32 or 64
    // (dynamic LDS, sized by the step: per 16-lane group and round one 64-bit mask and one round number - only the rounds with a
    // match are kept - and three words per row: 88 KB at kScanMaxRows)
    uint64_t *mask_all = reinterpret_cast<uint64_t *>(scan_lds);                      // [64 groups][rounds]
    uint32_t *key_s = reinterpret_cast<uint32_t *>(mask_all + (size_t)gpb * rounds);    // this side's table row of a step row
    uint32_t *oth_s = key_s + rounds * 64;                                            // the other side's
    float *dp_s = reinterpret_cast<float *>(oth_s + rounds * 64);
    uint16_t *rnd_all = reinterpret_cast<uint16_t *>(dp_s + rounds * 64);             // [64 groups][rounds]
    // (the norms first: their loads fly with the ids' - read after the scan they were a memory round trip of their own)
    const double nrm_m = stats[DAISY_NST_NORM + (side ? 3 : 1)], nrm_g = stats[DAISY_NST_NORM + (side ? 2 : 0)], nrm_neg = stats[DAISY_NST_NORM + 4];
    for (int t = tid; t < rounds * 64; t += (int)blockDim.x) {
        uint32_t own = 0xFFFFFFFFu, oth = 0u;
        float dp = 0.f;
        if (t < R) {
            int64_t user, item;
            pair_ids(src, t, user, item);
            own = (uint32_t)(side ? item : user);
            oth = (uint32_t)(side ? user : item);
            dp = dpred[t];
        }
        key_s[t] = own; oth_s[t] = oth; dp_s[t] = dp;
    }
    __syncthreads();
    SCAN_MARK(0)
    const int lane = tid % 16, group = tid / 16;
    // The scan: a wave compares 64 keys per round with the keys of ITS four rows - one LDS read, four compares, four ballots,
    // and a ballot IS the round's mask of matching rows; four rounds' reads are issued together (a round on its own is one LDS
    // latency: 22 us for 4096 rows).  Rounds without a match are not kept; the occurrence counts of the regulariser
    // (rows < B: positives) are taken from the masks as they pass.  A row with a match before itself is not the first occurrence
    // of its key: it owns nothing.
    __shared__ int cnt_s[kScatterSmallRows / 16], npos_s[kScatterSmallRows / 16], nneg_s[kScatterSmallRows / 16];
    {
        constexpr int Q = kWave / 16;
        // (the wave's number through readfirstlane: everything derived from it - its rows, their flags and counters - is then
        // scalar for the compiler too; as lane-derived values they were carried in VGPRs with exec-mask branches around
        // every step, ~110 instructions per round and row)
        const int lane64 = tid % kWave, wave = __builtin_amdgcn_readfirstlane(tid / kWave);
        const int g0 = wave * Q, e0 = (int)blockIdx.y * gpb + g0;
        uint32_t rowk[Q];
        int cnt[Q], np_[Q], nn_[Q];
        bool early[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) { rowk[q] = key_s[(e0 + q < R) ? e0 + q : 0]; cnt[q] = 0; np_[q] = 0; nn_[q] = 0; early[q] = e0 + q >= R; }
        for (int rb = 0; rb < rounds; rb += 4) {
            uint32_t kk[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) kk[x] = (rb + x < rounds) ? key_s[(rb + x) * 64 + lane64] : 0xFFFFFFFEu;
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int rd = rb + x;
                if (rd >= rounds) break;
                uint64_t mq[Q], any = 0;
#pragma unroll
                for (int q = 0; q < Q; ++q) { mq[q] = __ballot(kk[x] == rowk[q]); any |= mq[q]; }
                if (any == 0) continue;                                               // (most rounds: one branch for the four rows)
                const int64_t npos_bits = (int64_t)src.B - (int64_t)rd * 64;          // positions of this round that are positive rows
                const uint64_t posm = npos_bits >= 64 ? ~0ull : (npos_bits <= 0 ? 0ull : (((uint64_t)1 << npos_bits) - 1));
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const uint64_t m = mq[q];
                    if (m == 0 || early[q]) continue;
                    const int before = e0 + q - rd * 64;                              // positions of this round before the row itself
                    if (before >= 64 || (before > 0 && (m & (((uint64_t)1 << before) - 1)) != 0)) { early[q] = true; continue; }
                    if (lane64 == 0) { mask_all[(size_t)(g0 + q) * rounds + cnt[q]] = m; rnd_all[(size_t)(g0 + q) * rounds + cnt[q]] = (uint16_t)rd; }
                    ++cnt[q];
                    np_[q] += (int)__popcll(m & posm);
                    nn_[q] += (int)__popcll(m & ~posm);
                }
            }
        }
        if (lane64 == 0)
#pragma unroll
            for (int q = 0; q < Q; ++q) { cnt_s[g0 + q] = early[q] ? -1 : cnt[q]; npos_s[g0 + q] = np_[q]; nneg_s[g0 + q] = nn_[q]; }
    }
    // (the wave that wrote a row's masks is the wave its 16-lane group belongs to: no workgroup barrier)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    SCAN_MARK(1)
    const int e = (int)blockIdx.y * gpb + group;
    if (e >= R) return;
    const int nent = cnt_s[group];
    if (nent < 0) return;                                   // the first occurrence owns the table row
    const uint32_t row = key_s[e];
    const uint64_t *mask_s = mask_all + (size_t)group * rounds;       // this group's kept rounds: masks and round numbers
    const uint16_t *rnd_s = rnd_all + (size_t)group * rounds;
    const float npos = (float)npos_s[group], nneg = (float)nneg_s[group];
    SCAN_MARK(2)
    auto inv = [&](double n) { return (n > 0.0) ? (float)((double)reg_2 / n) : 0.f; };
    const float i_m = inv(nrm_m), i_g = inv(nrm_g), i_neg = 2.f * inv(nrm_neg);
    const float *tabM = side ? p.iM : p.uM, *tabG = side ? p.iG : p.uG, *otherG = side ? p.uG : p.iG;
    float *gM = side ? g.iM : g.uM, *gG = side ? g.iG : g.uG;
    // The table row's dm + d columns as float4 chunks, NT per lane, all of a step row's chunks loaded at once: one dependent
    // memory access (0.2 - 0.4 us: profiles/r06_latency_probe.txt) per matching step row plus one for the table rows and the
    // gradient rows, instead of three per 16 columns (first version: 20 us at factors 24, this one 10.5).  Per element the same operations
    // in the same order as k_nmf_scatter_small.
    const int mch = dm / 4, nch = mch + d / 4;         // chunks 0 .. mch-1: the MLP row; mch .. nch-1: the GMF row
    float4 acc[NT], tw[NT], gw[NT], wpv[NT <= 2 ? NT : 1];     // (NT = 5: 128 registers per lane at 1024 threads - Wp is read late there)
    int cidx[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int ch = lane + 16 * t;
        cidx[t] = (ch < nch) ? ch : -1;
        acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        const int cc = (ch < nch) ? ch : 0;
        const float *trow = (cc < mch) ? tabM + (int64_t)row * dm + 4 * cc : tabG + (int64_t)row * d + 4 * (cc - mch);
        const float *grow_ = (cc < mch) ? gM + (int64_t)row * dm + 4 * cc : gG + (int64_t)row * d + 4 * (cc - mch);
        tw[t] = *reinterpret_cast<const float4 *>(trow);
        gw[t] = *reinterpret_cast<const float4 *>(grow_);
        if constexpr (NT <= 2) wpv[t] = *reinterpret_cast<const float4 *>(p.Wp + ((cc < mch) ? 0 : 4 * (cc - mch)));
    }
    for (int c = 0; c < nent; ++c)
        for (uint64_t m = mask_s[c]; m; m &= m - 1) {
            const int r = (int)rnd_s[c] * 64 + (int)__builtin_ctzll(m);
            const float dp = dp_s[r];
            const float *xrow = DX0 + (int64_t)r * (2 * dm) + side * dm, *orow = otherG + (int64_t)oth_s[r] * d;
            float4 v[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int cc = cidx[t] < 0 ? 0 : cidx[t];
                v[t] = *reinterpret_cast<const float4 *>((cc < mch) ? xrow + 4 * cc : orow + 4 * (cc - mch));
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (cidx[t] < 0) continue;
                if (cidx[t] < mch) {
                    if (model != DAISY_NEUMF_GMF) { acc[t].x += v[t].x; acc[t].y += v[t].y; acc[t].z += v[t].z; acc[t].w += v[t].w; }
                } else if (model != DAISY_NEUMF_MLP) {
                    acc[t].x = fmaf(dp, v[t].x, acc[t].x); acc[t].y = fmaf(dp, v[t].y, acc[t].y);
                    acc[t].z = fmaf(dp, v[t].z, acc[t].z); acc[t].w = fmaf(dp, v[t].w, acc[t].w);
                }
            }
        }
    SCAN_MARK(3)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (cidx[t] < 0) continue;
        float a4[4] = {acc[t].x, acc[t].y, acc[t].z, acc[t].w};
        const float w4[4] = {tw[t].x, tw[t].y, tw[t].z, tw[t].w};
        float o4[4] = {gw[t].x, gw[t].y, gw[t].z, gw[t].w};
        if (cidx[t] < mch) {
            // MLP table: the rows' input gradients (this side's half of dX0), the regulariser on the positive rows' occurrences
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float v = a4[k];
                if (npos > 0.f) v += fmaf(npos * i_m, w4[k], reg_1 * npos * sgn(w4[k]));
                if (v != 0.f) o4[k] += v;
            }
            *reinterpret_cast<float4 *>(gM + (int64_t)row * dm + 4 * cidx[t]) = make_float4(o4[0], o4[1], o4[2], o4[3]);
        } else {
            // GMF table: Wp[c] x sum of dpred[r] x the OTHER table's row; the negative item's rows count twice in the regulariser
            const int c0 = 4 * (cidx[t] - mch);
            float4 wq;
            if constexpr (NT <= 2) wq = wpv[t]; else wq = *reinterpret_cast<const float4 *>(p.Wp + c0);
            const float wp4[4] = {wq.x, wq.y, wq.z, wq.w};
            const float na = npos, nb = (side && !pointwise) ? nneg : 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float v = a4[k];
                if (model != DAISY_NEUMF_MLP) v *= wp4[k];
                if (na + nb > 0.f) v += fmaf(na * i_g + nb * i_neg, w4[k], reg_1 * (na + 2.f * nb) * sgn(w4[k]));
                if (v != 0.f) o4[k] += v;
            }
            *reinterpret_cast<float4 *>(gG + (int64_t)row * d + c0) = make_float4(o4[0], o4[1], o4[2], o4[3]);
        }
    }
#ifdef DAISY_SCAN_PROF
    SCAN_MARK(4)
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0)
        printf("k_nmf_scatter_scan block 0 group 0, x10 ns: ids->LDS %lld  scan %lld  counts %lld  table rows + matches %lld  commit %lld (R %d)\n",
               sprof[0], sprof[1], sprof[2], sprof[3], sprof[4], R);
#endif
}

// ---------------------------------------------------------------------------------------------
// Round 6: the step's rows grouped by user and by item with ONE stable counting pass per side instead of two radix sorts
// (rocprim: two digit passes + histogram + ~5 memsets per sort - 88 us per side at 524 288 rows, a launch chain, not
// bandwidth).  The table has a few thousand rows (ml-1m: 6040 / 3706), so a whole histogram fits a wave's share of LDS:
//   k_cs_count    each wave counts the keys of ITS contiguous range of rows (LDS atomics: counts do not depend on order)
//   k_cs_prefix   per key: exclusive prefix over the waves' counts, in wave order (= row order); the pos / neg halves' totals
//                 are the regulariser's occurrence counts (what k_nmf_sort_keys counted with global atomics)
//   k_cs_base     exclusive scan of the keys' totals
//   k_cs_entries  the slots' rows -> the segmented reductions' entry lists, with coalesced stores
//   k_cs_scatter  each wave walks its rows in order, 64 at a time: a row's slot = base[key] + the waves before + the rows of
//                 this wave before it with the same key (ballot match inside the 64, a running LDS counter across them)
// Stable by construction - rows of one key stay in ascending row order - hence the same bits as the radix sorts' output.
// Both sides (users, items) ride in the same four launches (blockIdx.y).
// ---------------------------------------------------------------------------------------------
constexpr int kCsBlocks = 128, kCsWaves = kBlock / kWave, kCsNW = kCsBlocks * kCsWaves;      // 512 wave ranges per side
constexpr int kCsMaxKeys = 9600;                                                             // 4 waves x keys x 4 B <= 150 KB of LDS

struct CsRange { int64_t lo, hi; };
// wave range gw of a step of R rows: the pos half [0, B) and the neg half [B, R) are cut separately (so that a half's counts
// are whole waves); point-wise steps have one half
__device__ __forceinline__ CsRange cs_range(int gw, int64_t R, int64_t B, int halves) {
    const int wph = kCsNW / halves, hf = gw / wph, within = gw % wph;
    const int64_t len = (halves == 2) ? ((hf == 0) ? B : R - B) : R, base = (halves == 2 && hf == 1) ? B : 0;
    const int64_t chunk = ((len + wph - 1) / wph + kWave - 1) / kWave * kWave;
    int64_t lo = base + within * chunk, hi = lo + chunk;
    if (lo > base + len) lo = base + len;
    if (hi > base + len) hi = base + len;
    return CsRange{lo, hi};
}
__device__ __forceinline__ int32_t cs_key(const PairSrc &src, int64_t r, int side) {
    int64_t user, item;
    pair_ids(src, r, user, item);
    return (int32_t)(side ? item : user);
}

__global__ __launch_bounds__(kBlock) void k_cs_count(PairSrc src, int64_t R, int halves, int Ku, int Ki, int kstride,
                                                     int32_t *__restrict__ hist) {
    extern __shared__ int32_t cs_lds[];
    const int side = blockIdx.y, K = side ? Ki : Ku;
    // (the wave's number through readfirstlane: its range and the loops over it are then scalar for the compiler too)
    const int lane = threadIdx.x % kWave, w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), gw = blockIdx.x * kCsWaves + w;
    int32_t *h = cs_lds + w * kstride;
    for (int k = lane; k < K; k += kWave) h[k] = 0;
    const CsRange rg = cs_range(gw, R, src.B, halves);
    for (int64_t r0 = rg.lo + lane; r0 < rg.hi; r0 += 4 * kWave) {          // four rows' ids in flight per lane
        int32_t key[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) key[x] = (r0 + x * kWave < rg.hi) ? cs_key(src, r0 + x * kWave, side) : -1;
#pragma unroll
        for (int x = 0; x < 4; ++x) if (key[x] >= 0) atomicAdd(&h[key[x]], 1);
    }
    // (a wave's LDS operations complete in order: no barrier between its own adds and reads)
    int32_t *out = hist + ((int64_t)side * kCsNW + gw) * kstride;
    for (int k = lane; k < K; k += kWave) out[k] = h[k];
}

__global__ __launch_bounds__(kBlock) void k_cs_prefix(int halves, int Ku, int Ki, int kstride, int32_t *__restrict__ hist,
                                                      int32_t *__restrict__ total, int32_t *__restrict__ cnt_u,
                                                      int32_t *__restrict__ cnt_i, int32_t *__restrict__ cnt_j) {
    const int side = blockIdx.y, K = side ? Ki : Ku;
    const int key = blockIdx.x * kBlock + threadIdx.x;
    if (key >= K) return;
    int32_t *col = hist + (int64_t)side * kCsNW * kstride + key;
    const int wph = kCsNW / halves;
    int32_t run = 0, first_half = 0;
    static_assert(kCsNW % 64 == 0, "the prefix walks the wave ranges 32 at a time, and a half is a whole number of such groups");
    for (int g0 = 0; g0 < kCsNW; g0 += 32) {                    // 32 independent loads in flight (8: 64 dependent round trips, 28 us), then the running sum
        int32_t cnt[32];
#pragma unroll
        for (int x = 0; x < 32; ++x) cnt[x] = col[(int64_t)(g0 + x) * kstride];
#pragma unroll
        for (int x = 0; x < 32; ++x) { col[(int64_t)(g0 + x) * kstride] = run; run += cnt[x]; }
        if (g0 + 32 == wph) first_half = run;
    }
    if (halves == 1) first_half = run;
    total[side * kstride + key] = run;
    // the regulariser's occurrence counts (NeuMFRecommender.py:149-167): users / items of the positive rows, items of the negatives
    if (side == 0) cnt_u[key] = first_half;
    else { cnt_i[key] = first_half; cnt_j[key] = run - first_half; }
}

// exclusive scan of total[side][0 .. K) in place (one workgroup per side; K <= kCsMaxKeys)
__global__ __launch_bounds__(1024) void k_cs_base(int Ku, int Ki, int kstride, int32_t *__restrict__ total) {
    __shared__ int32_t part[1024];
    const int side = blockIdx.x, K = side ? Ki : Ku, tid = threadIdx.x;
    int32_t *t = total + side * kstride;
    const int per = (K + 1023) / 1024, lo = tid * per, hi = (lo + per < K) ? lo + per : K;
    int32_t sum = 0;
    for (int k = lo; k < hi; ++k) sum += t[k];
    part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {                 // Hillis-Steele over the 1024 partial sums
        const int32_t v = (tid >= off) ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int32_t run = part[tid] - sum;                             // exclusive
    for (int k = lo; k < hi; ++k) { const int32_t c = t[k]; t[k] = run; run += c; }
}

// The grouped rows leave as the segmented reduction's entry lists (what k_nmf_entries / k_nmf_entries_gmf wrote in four launches
// of their own): per side, entry e -> key = table row << 1; MLP list: source row = mlp_rows_per * r + half, weight 1; GMF list:
// source row = the OTHER id of row r, weight dpred[r].  An odd count is padded with a weightless copy of the last entry.
struct CsEntries { uint32_t *ekey; uint2 *esu_m; float2 *w_m; uint2 *esu_g; float2 *w_g; };
__global__ __launch_bounds__(kBlock) void k_cs_scatter(PairSrc src, int64_t R, int halves, int Ku, int Ki, int kstride,
                                                       const int32_t *__restrict__ hist, const int32_t *__restrict__ total,
                                                       CsEntries eu, CsEntries ei, int mlp_rows_per, int mlp_half_by_side,
                                                       const float *__restrict__ dpred) {
    extern __shared__ int32_t cs_lds[];
    const int side = blockIdx.y, K = side ? Ki : Ku;
    const int lane = threadIdx.x % kWave, w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), gw = blockIdx.x * kCsWaves + w;
    int32_t *off = cs_lds + w * kstride;
    const int32_t *mine = hist + ((int64_t)side * kCsNW + gw) * kstride, *base = total + side * kstride;
    for (int k = lane; k < K; k += kWave) off[k] = base[k] + mine[k];
    const CsEntries en = side ? ei : eu;
    (void)mlp_rows_per; (void)mlp_half_by_side; (void)dpred;          // (the entries themselves: k_cs_entries)
    const CsRange rg = cs_range(gw, R, src.B, halves);
    const uint64_t lt = ((uint64_t)1 << lane) - 1;
    for (int64_t rb = rg.lo; rb < rg.hi; rb += 4 * kWave) {
      int32_t keys[4];                                         // the ids of four 64-row groups in flight
#pragma unroll
      for (int x = 0; x < 4; ++x) keys[x] = (rb + x * kWave + lane < rg.hi) ? cs_key(src, rb + x * kWave + lane, side) : -1;
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int64_t r = rb + x * kWave + lane;
        const bool valid = r < rg.hi;
        const int32_t key = keys[x];
        if (rb + x * kWave >= rg.hi) break;
        uint64_t peers = __ballot(valid);                      // lanes of this 64 with the same key
#pragma unroll
        for (int b = 0; b < 14; ++b) {
            const uint64_t m = __ballot((key >> b) & 1);
            peers &= ((key >> b) & 1) ? m : ~m;
        }
        if (valid) {
            // the row's number into its slot (ONE scattered 4-byte store per row; k_cs_entries turns the slots into entries with
            // coalesced stores - writing the five entry arrays from here was five scattered partial-line stores per row: 83 us)
            const int32_t slot = off[key] + (int32_t)__popcll(peers & lt);
            en.ekey[slot] = (uint32_t)r;
            if ((peers & lt) == 0) off[key] += (int32_t)__popcll(peers);      // one lane per key moves the running counter
        }
      }
    }
}

// slot e of a side (holding the step row k_cs_scatter put there) -> the segmented reductions' entries, both lists
__global__ __launch_bounds__(kBlock) void k_cs_entries(PairSrc src, int64_t R, CsEntries eu, CsEntries ei, int mlp_rows_per,
                                                       int mlp_half_by_side, const float *__restrict__ dpred) {
    const int side = blockIdx.y;
    const CsEntries en = side ? ei : eu;
    const int half = mlp_half_by_side ? side : 0;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < R; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = en.ekey[e];
        int64_t user, item;
        pair_ids(src, r, user, item);
        const uint32_t ek = (uint32_t)(side ? item : user) << 1, sm = (uint32_t)(mlp_rows_per * (int32_t)r + half),
                       sg = (uint32_t)(side ? user : item);
        const float dp = dpred ? dpred[r] : 0.f;
        en.ekey[e] = ek;
        en.esu_m[e] = make_uint2((uint32_t)e, sm); en.w_m[e] = make_float2(1.f, 0.f);
        en.esu_g[e] = make_uint2((uint32_t)e, sg); en.w_g[e] = make_float2(dp, 0.f);
        if ((R & 1) && e == R - 1) {                       // the weightless copy that makes the count even
            en.ekey[R] = ek;
            en.esu_m[R] = make_uint2((uint32_t)R, sm); en.w_m[R] = make_float2(0.f, 0.f);
            en.esu_g[R] = make_uint2((uint32_t)R, sg); en.w_g[R] = make_float2(0.f, 0.f);
        }
    }
}

__global__ void k_nmf_sort_keys(PairSrc src, int64_t R, int32_t *__restrict__ ku, int32_t *__restrict__ ki,
                                int32_t *__restrict__ val, int pointwise, int32_t *__restrict__ cnt_u,
                                int32_t *__restrict__ cnt_i, int32_t *__restrict__ cnt_j) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x) {
        int64_t user, item;
        pair_ids(src, r, user, item);
        ku[r] = (int32_t)user;
        ki[r] = (int32_t)item;
        val[r] = (int32_t)r;
        if (r < src.B) { atomicAdd(cnt_u + user, 1); atomicAdd(cnt_i + item, 1); }     // regulariser occurrences (:149-167)
        else if (!pointwise) atomicAdd(cnt_j + item, 1);
    }
}

// entry e of a sorted list -> the segmented reduction's view: key = table row << 1, source row = rows_per*r + half
__global__ void k_nmf_entries(const int32_t *__restrict__ key_sorted, const int32_t *__restrict__ val_sorted, int64_t R,
                              int64_t n_pad, int rows_per, int half, uint32_t *__restrict__ ekey,
                              uint2 *__restrict__ esu, float2 *__restrict__ w) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n_pad; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = e < R ? e : R - 1;               // an odd count is padded with a weightless copy of the last entry
        ekey[e] = (uint32_t)key_sorted[q] << 1;
        esu[e] = make_uint2((uint32_t)e, (uint32_t)(rows_per * val_sorted[q] + half));
        w[e] = make_float2(e < R ? 1.f : 0.f, 0.f);
    }
}

// GMF branch: d/d uG[user] = Wp * sum over the user's rows of dpred[r] * iG[item_r]  (and the mirror image for iG).  The
// sum is a segmented reduction over the rows sorted by user whose SOURCE rows are the other table's - cache-resident - rows
// and whose weights are dpred[r]: entry e -> (key = table row << 1, source row = the other id of row r, weight dpred[r]);
// Wp multiplies the finished sum (k_nmf_table_commit).  Until round 5 the per-row products were materialised first (two
// [R, d] fp32 arrays written by a kernel of their own and read back by the reductions: 0.4 GB per step at R = 524 288).
__global__ void k_nmf_entries_gmf(const int32_t *__restrict__ key_sorted, const int32_t *__restrict__ val_sorted, int64_t R,
                                  int64_t n_pad, PairSrc src, int side, const float *__restrict__ dpred,
                                  uint32_t *__restrict__ ekey, uint2 *__restrict__ esu, float2 *__restrict__ w) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n_pad; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = e < R ? e : R - 1;               // an odd count is padded with a weightless copy of the last entry
        const int64_t r = val_sorted[q];
        int64_t user, item;
        pair_ids(src, r, user, item);
        ekey[e] = (uint32_t)key_sorted[q] << 1;
        esu[e] = make_uint2((uint32_t)e, (uint32_t)(side ? user : item));
        w[e] = make_float2(e < R ? dpred[r] : 0.f, 0.f);
    }
}

// g[row] += sum[row] (clearing sum) + (ca*ia + cb*ib) * w[row] + reg_1*(ca + cb) * sign(w[row]); counts cleared
__global__ __launch_bounds__(kBlock) void k_nmf_table_commit(float *__restrict__ g, float *__restrict__ sum,
                                                             const float *__restrict__ w, int64_t rows, int width,
                                                             int32_t *__restrict__ ca, int ka, int32_t *__restrict__ cb,
                                                             int kb, float scale_b, const double *__restrict__ stats,
                                                             float reg_1, float reg_2, int clear_counts,
                                                             const float *__restrict__ colscale = nullptr) {
    const int lane = threadIdx.x % 16, group = threadIdx.x / 16;
    const int64_t gstride = (int64_t)gridDim.x * (kBlock / 16);
    auto inv = [&](int k) { const double n = stats[DAISY_NST_NORM + k]; return (n > 0.0) ? (float)((double)reg_2 / n) : 0.f; };
    const float ia = inv(ka), ib = cb ? scale_b * inv(kb) : 0.f;
    for (int64_t row = (int64_t)blockIdx.x * (kBlock / 16) + group; row < rows; row += gstride) {
        const float na = (float)ca[row], nb = cb ? (float)cb[row] : 0.f;
        const float r2 = na * ia + nb * ib, r1 = reg_1 * (na + scale_b * nb);
        for (int c = lane; c < width; c += 16) {
            const int64_t x = row * (int64_t)width + c;
            float v = 0.f;
            if (sum) { v = colscale ? sum[x] * colscale[c] : sum[x]; sum[x] = 0.f; }      // (GMF tables: Wp x the summed rows)
            if (na + nb > 0.f) { const float e = w[x]; v += fmaf(r2, e, r1 * sgn(e)); }
            if (v != 0.f) g[x] += v;
        }
        if (clear_counts && lane == 0) { ca[row] = 0; if (cb) cb[row] = 0; }
    }
}

// the same with 16-byte accesses (width % 4 == 0, 16-byte aligned tables): a lane takes 4 consecutive columns - the scalar form
// above walks a 256-column row in 16 dependent trips per lane and cost 15-19 us per table for 6 MB
__global__ __launch_bounds__(kBlock) void k_nmf_table_commit_v(float *__restrict__ g, float *__restrict__ sum,
                                                               const float *__restrict__ w, int64_t rows, int width,
                                                               int32_t *__restrict__ ca, int ka, int32_t *__restrict__ cb,
                                                               int kb, float scale_b, const double *__restrict__ stats,
                                                               float reg_1, float reg_2, int clear_counts,
                                                               const float *__restrict__ colscale) {
    const int lane = threadIdx.x % 16, group = threadIdx.x / 16;
    const int64_t gstride = (int64_t)gridDim.x * (kBlock / 16);
    auto inv = [&](int k) { const double n = stats[DAISY_NST_NORM + k]; return (n > 0.0) ? (float)((double)reg_2 / n) : 0.f; };
    const float ia = inv(ka), ib = cb ? scale_b * inv(kb) : 0.f;
    for (int64_t row = (int64_t)blockIdx.x * (kBlock / 16) + group; row < rows; row += gstride) {
        const float na = (float)ca[row], nb = cb ? (float)cb[row] : 0.f;
        const float r2 = na * ia + nb * ib, r1 = reg_1 * (na + scale_b * nb);
        const bool reg = na + nb > 0.f;
        if (!sum && !reg) continue;
        for (int c = 4 * lane; c < width; c += 64) {
            const int64_t x = row * (int64_t)width + c;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (sum) {
                const float4 sv = *reinterpret_cast<const float4 *>(sum + x);
                v[0] = sv.x; v[1] = sv.y; v[2] = sv.z; v[3] = sv.w;
                if (colscale) {
                    const float4 cs = *reinterpret_cast<const float4 *>(colscale + c);
                    v[0] *= cs.x; v[1] *= cs.y; v[2] *= cs.z; v[3] *= cs.w;
                }
                *reinterpret_cast<float4 *>(sum + x) = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            if (reg) {
                const float4 ev = *reinterpret_cast<const float4 *>(w + x);
                const float e[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] += fmaf(r2, e[k], r1 * sgn(e[k]));
            }
            float4 gv = *reinterpret_cast<float4 *>(g + x);
            gv.x += v[0]; gv.y += v[1]; gv.z += v[2]; gv.w += v[3];      // (+ 0 where nothing arrived: the bits of g stay)
            *reinterpret_cast<float4 *>(g + x) = gv;
        }
        if (clear_counts && lane == 0) { ca[row] = 0; if (cb) cb[row] = 0; }
    }
}

// Both tables of a side - MLP then GMF - for both sides in ONE launch (blockIdx.y: the side): the four commits of a step were
// four launches of ~6.5 us each, mostly latency.  A lane group takes a table row of its side and commits its MLP row, its GMF
// row, then clears the row's occurrence counts (both commits read them).  Per element the operations of k_nmf_table_commit_v.
struct CommitSide {
    float *gM, *sumM; const float *wM; int widthM, kM;            // MLP table: gradient, row sums (or null), weights, columns, norm slot
    float *gG, *sumG; const float *wG; int widthG, kG;            // GMF table
    int64_t rows;
    int32_t *ca, *cb;                                             // occurrences: positives; negatives (items' GMF rows only, or null)
    const float *colscale;                                        // Wp over the GMF sums (or null)
};
__global__ __launch_bounds__(kBlock) void k_nmf_table_commit_pair(CommitSide su, CommitSide si, const double *__restrict__ stats,
                                                                  float reg_1, float reg_2) {
    const CommitSide &j = blockIdx.y ? si : su;
    const int lane = threadIdx.x % 16, group = threadIdx.x / 16;
    const int64_t gstride = (int64_t)gridDim.x * (kBlock / 16);
    auto inv = [&](int k) { const double n = stats[DAISY_NST_NORM + k]; return (n > 0.0) ? (float)((double)reg_2 / n) : 0.f; };
    const float iM = inv(j.kM), iG = inv(j.kG), iN = j.cb ? 2.f * inv(4) : 0.f;
    for (int64_t row = (int64_t)blockIdx.x * (kBlock / 16) + group; row < j.rows; row += gstride) {
        const float na = (float)j.ca[row], nb = j.cb ? (float)j.cb[row] : 0.f;
        auto commit = [&](float *g, float *sum, const float *w, int width, float r2, float r1, bool reg, const float *colscale) {
            if (!sum && !reg) return;
            for (int c = 4 * lane; c < width; c += 64) {
                const int64_t x = row * (int64_t)width + c;
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                if (sum) {
                    const float4 sv = *reinterpret_cast<const float4 *>(sum + x);
                    v[0] = sv.x; v[1] = sv.y; v[2] = sv.z; v[3] = sv.w;
                    if (colscale) {
                        const float4 cs = *reinterpret_cast<const float4 *>(colscale + c);
                        v[0] *= cs.x; v[1] *= cs.y; v[2] *= cs.z; v[3] *= cs.w;
                    }
                    *reinterpret_cast<float4 *>(sum + x) = make_float4(0.f, 0.f, 0.f, 0.f);
                }
                if (reg) {
                    const float4 ev = *reinterpret_cast<const float4 *>(w + x);
                    const float e[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] += fmaf(r2, e[k], r1 * sgn(e[k]));
                }
                float4 gv = *reinterpret_cast<float4 *>(g + x);
                gv.x += v[0]; gv.y += v[1]; gv.z += v[2]; gv.w += v[3];      // (+ 0 where nothing arrived: the bits of g stay)
                *reinterpret_cast<float4 *>(g + x) = gv;
            }
        };
        // (k_nmf_table_commit_v's r2 = na * ia + nb * ib, r1 = reg_1 * (na + scale_b * nb) with ib = scale_b * inv(kb))
        commit(j.gM, j.sumM, j.wM, j.widthM, na * iM + 0.f * 0.f, reg_1 * (na + 0.f * 0.f), na + 0.f > 0.f, nullptr);
        commit(j.gG, j.sumG, j.wG, j.widthG, na * iG + nb * iN, reg_1 * (na + 2.f * nb), na + nb > 0.f, j.colscale);
        if (lane == 0) { j.ca[row] = 0; if (j.cb) j.cb[row] = 0; }
    }
}

static void launch_table_commit(float *g, float *sum, const float *w, int64_t rows, int width, int32_t *ca, int ka, int32_t *cb,
                                int kb, float scale_b, const double *stats, float reg_1, float reg_2, int clear_counts,
                                const float *colscale, hipStream_t s) {
    auto al = [](const void *p) { return p == nullptr || ((uintptr_t)p & 15) == 0; };
    if (width % 4 == 0 && al(g) && al(sum) && al(w) && al(colscale))
        hipLaunchKernelGGL(k_nmf_table_commit_v, dim3(grid_for(rows, kBlock / 16)), dim3(kBlock), 0, s, g, sum, w, rows, width, ca, ka,
                           cb, kb, scale_b, stats, reg_1, reg_2, clear_counts, colscale);
    else
        hipLaunchKernelGGL(k_nmf_table_commit, dim3(grid_for(rows, kBlock / 16 * 2)), dim3(kBlock), 0, s, g, sum, w, rows, width, ca,
                           ka, cb, kb, scale_b, stats, reg_1, reg_2, clear_counts, colscale);
}

// the owner chain's scratch, at its first use
static int neumf_scatter_scratch(NeumfScatter &c) {
    if (c.arena.bytes()) return DAISY_OK;
    const size_t R = (size_t)c.max_rows + 1, dm = (size_t)c.dm;
    const size_t rows_max = (size_t)(c.U > c.I ? c.U : c.I);
    size_t chunks = (size_t)segsum_chunks((int64_t)R + 1, c.dm);
    const size_t ch2 = (size_t)segsum_chunks((int64_t)R + 1, c.d);
    if (ch2 > chunks) chunks = ch2;
    chunks += 2;
    c.tmp_bytes = sort_pairs_i32_temp_bytes_upto((int64_t)R);
    DeviceArena &a = c.arena;
    a.add(&c.ku, R * 4); a.add(&c.ki, R * 4); a.add(&c.val, R * 4); a.add(&c.ks, R * 4); a.add(&c.vs, R * 4);
    a.add(&c.cu, (size_t)c.U * 4); a.add(&c.ci, (size_t)c.I * 4); a.add(&c.cj, (size_t)c.I * 4);
    a.add(&c.ekey, (R + 1) * 4); a.add(&c.esu, (R + 1) * 8); a.add(&c.w, (R + 1) * 8);
    a.add(&c.sum, rows_max * dm * 4); a.add(&c.sum2, rows_max * dm * 4);
    a.add(&c.sumg, rows_max * (size_t)c.d * 4); a.add(&c.sumg2, rows_max * (size_t)c.d * 4);
    a.add(&c.edge_vec, 2 * chunks * dm * 4); a.add(&c.edge_item, 2 * chunks * 4); a.add(&c.edge_b, 2 * chunks * 4);
    a.add(&c.edge_whole, chunks * 4);
    a.add(&c.tmp, c.tmp_bytes);
    if (int rc = a.alloc("neumf: the scatter scratch")) {
        a.release();
        return rc;
    }
    // the counts and the row-sum table are kept all-zero between calls by the kernels that consume them
    // (the three count arrays are adjacent slots, and so are the four sum tables)
    hipError_t e = hipMemset(c.cu, 0, (size_t)((char *)c.ekey - (char *)c.cu));
    if (e == hipSuccess) e = hipMemset(c.sum, 0, (size_t)((char *)c.sumg2 - (char *)c.sum) + rows_max * (size_t)c.d * 4);
    if (e != hipSuccess) { a.release(); set_error("neumf: hipMemset of the scatter scratch failed"); return DAISY_ERR_HIP; }
    return DAISY_OK;
}

static CsEntries cs_entries(const NeumfScatter &c, int side) {
    const size_t per = align_up(((size_t)c.max_rows + 2) * 8);
    char *b = (char *)c.cs_ent + (size_t)side * 5 * per;
    return CsEntries{(uint32_t *)b, (uint2 *)(b + per), (float2 *)(b + 2 * per), (uint2 *)(b + 3 * per), (float2 *)(b + 4 * per)};
}

int neumf_scatter(NeumfScatter &c, const NeumfPath &path, const daisy_neumf_params &p, const daisy_neumf_params &g,
                  const PairSrc &src, int64_t R, int pointwise, const float *dpred, const float *DX0, const double *stats,
                  float reg_1, float reg_2, hipStream_t s) {
    const bool dx0_bf16 = path.H, fact = path.fact;
    {
        // small steps: the whole scatter in one launch (k_nmf_scatter_scan).  DAISY_NMF_SCATTER_SMALL (read per call): 0 - off,
        // 2 - the sorting kernel it replaced (k_nmf_scatter_small: A/B, and the tests' bit-for-bit cross-check)
        const char *env_sm = getenv("DAISY_NMF_SCATTER_SMALL");
        const int sm_mode = env_sm ? atoi(env_sm) : 1;
        // (the scanning kernel holds a table row's dm + d columns as 16 x 5 float4 at most; 16-byte aligned tables and gradients)
        const bool scan_ok = (c.dm + c.d) / 4 <= 80 &&
                             ((((uintptr_t)p.uM | (uintptr_t)p.iM | (uintptr_t)p.uG | (uintptr_t)p.iG | (uintptr_t)g.uM | (uintptr_t)g.iM |
                                (uintptr_t)g.uG | (uintptr_t)g.iG | (uintptr_t)DX0 | (uintptr_t)p.Wp) & 15) == 0);
        const bool sort_ok = R <= kScatterSmallRows && c.U < (1 << 22) && c.I < (1 << 22);
        if (R <= kScanMaxRows && !dx0_bf16 && !fact && sm_mode != 0 && (scan_ok || sort_ok)) {
            if ((sm_mode == 2 || !scan_ok) && sort_ok)
                hipLaunchKernelGGL(k_nmf_scatter_small, dim3(2, 16), dim3(kScatterSmallRows), 0, s, p, g, src, (int)R, c.d, c.dm, c.model,
                                   pointwise, dpred, DX0, stats, reg_1, reg_2);
            else if (scan_ok) {
                const int blk = scan_block(R), gpb = blk / 16;
                const dim3 grid(2, (unsigned)((R + gpb - 1) / gpb));
                const int nt = ((c.dm + c.d) / 4 + 15) / 16;          // float4 chunks of a table row's columns per lane
                const int rounds = (int)((R + 63) / 64);
                const size_t lds = (size_t)gpb * rounds * 10 + (size_t)rounds * 64 * 12;
                static bool attr_set = false;
                if (!attr_set) {
                    const int cap = (scan_block(kScanMaxRows) / 16) * (kScanMaxRows / 64) * 10 + kScanMaxRows * 12;
                    DAISY_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_nmf_scatter_scan<2>), hipFuncAttributeMaxDynamicSharedMemorySize, cap));
                    DAISY_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_nmf_scatter_scan<5>), hipFuncAttributeMaxDynamicSharedMemorySize, cap));
                    attr_set = true;
                }
                if (nt <= 2) hipLaunchKernelGGL((k_nmf_scatter_scan<2>), grid, dim3(blk), lds, s, p, g, src, (int)R, c.d, c.dm,
                                                c.model, pointwise, dpred, DX0, stats, reg_1, reg_2);
                else hipLaunchKernelGGL((k_nmf_scatter_scan<5>), grid, dim3(blk), lds, s, p, g, src, (int)R, c.d, c.dm,
                                        c.model, pointwise, dpred, DX0, stats, reg_1, reg_2);
            } else {
                set_error("neumf: no small-step scatter for this step (rows %lld)", (long long)R);
                return DAISY_ERR_STATE;
            }
            DAISY_LAUNCH_CHECK();
            return DAISY_OK;
        }
    }
    int rc = neumf_scatter_scratch(c);
    if (rc) return rc;
    const int d = c.d, dm = c.dm, model = c.model;
    const int64_t n_pad = R + (R & 1);
    // rows grouped by table row: the counting pass (tables of at most kCsMaxKeys rows - a histogram per wave fits the LDS),
    // else two radix sorts.  DAISY_NMF_COUNTING=0 (read per call): always the sorts (A/B, and the tests' cross-check)
    const char *env_cs = getenv("DAISY_NMF_COUNTING");
    const int Kmax = (int)(c.U > c.I ? c.U : c.I);
    const bool counting = (!env_cs || atoi(env_cs) != 0) && Kmax <= kCsMaxKeys && Kmax < (1 << 14) && R >= 4096;
    const int kstride = (Kmax + 63) / 64 * 64;
    if (counting) {
        if (!c.cs_arena.bytes()) {             // the histograms and the entry lists: one allocation, so both or neither
            const size_t per = align_up(((size_t)c.max_rows + 2) * 8);       // one array of (rows + pad) x 8 bytes
            c.cs_arena.add(&c.cs_hist, (size_t)2 * (kCsNW + 1) * (size_t)((kCsMaxKeys + 63) / 64 * 64) * sizeof(int32_t));
            c.cs_arena.add(&c.cs_ent, 2 * 5 * per);
            if (int rc_cs = c.cs_arena.alloc("neumf: the counting pass's histograms and entry lists")) {
                c.cs_arena.release();
                return rc_cs;
            }
        }
        static bool cs_attr_set = false;       // (tied to the calls having succeeded, not to the buffers)
        if (!cs_attr_set) {
            DAISY_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_cs_count), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096));
            DAISY_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_cs_scatter), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096));
            cs_attr_set = true;
        }
        const int halves = pointwise ? 1 : 2;
        int32_t *total = c.cs_hist + (size_t)2 * kCsNW * kstride;
        const size_t lds = (size_t)kCsWaves * kstride * sizeof(int32_t);
        hipLaunchKernelGGL(k_cs_count, dim3(kCsBlocks, 2), dim3(kBlock), lds, s, src, R, halves, (int)c.U, (int)c.I, kstride, c.cs_hist);
        hipLaunchKernelGGL(k_cs_prefix, dim3((Kmax + kBlock - 1) / kBlock, 2), dim3(kBlock), 0, s, halves, (int)c.U, (int)c.I, kstride,
                           c.cs_hist, total, c.cu, c.ci, c.cj);
        hipLaunchKernelGGL(k_cs_base, dim3(2), dim3(1024), 0, s, (int)c.U, (int)c.I, kstride, total);
        hipLaunchKernelGGL(k_cs_scatter, dim3(kCsBlocks, 2), dim3(kBlock), lds, s, src, R, halves, (int)c.U, (int)c.I, kstride,
                           c.cs_hist, total, cs_entries(c, 0), cs_entries(c, 1), fact ? 1 : 2, fact ? 0 : 1,
                           (const float *)dpred);
        hipLaunchKernelGGL(k_cs_entries, dim3(grid_for(R, kBlock, 2048), 2), dim3(kBlock), 0, s, src, R, cs_entries(c, 0), cs_entries(c, 1),
                           fact ? 1 : 2, fact ? 0 : 1, (const float *)dpred);
    } else {
        hipLaunchKernelGGL(k_nmf_sort_keys, dim3(grid_for(R, kBlock * 2)), dim3(kBlock), 0, s, src, R, c.ku, c.ki,
                           c.val, pointwise, c.cu, c.ci, c.cj);
    }
    DAISY_LAUNCH_CHECK();
    // both sides' commits in one launch (k_nmf_table_commit_pair) when every operand takes float4 accesses; each side then has row-sum
    // tables of its own (a shared one had to be committed before the other side's reduction refilled it)
    auto al16 = [](const void *q) { return q == nullptr || ((uintptr_t)q & 15) == 0; };
    const bool pair_commit = dm % 4 == 0 && d % 4 == 0 && al16(g.uM) && al16(g.iM) && al16(g.uG) && al16(g.iG) && al16(p.uM) && al16(p.iM) &&
                             al16(p.uG) && al16(p.iG) && al16(p.Wp);
    CommitSide cside[2];
    for (int side = 0; side < 2; ++side) {            // 0: the user tables, 1: the item tables
        const int64_t rows = side ? c.I : c.U;
        float *sumM = side ? c.sum2 : c.sum, *sumG = side ? c.sumg2 : c.sumg;
        // the side's grouped rows: (keys, row ids) in table-row order, rows ascending inside a key
        const int32_t *g_ks = c.ks, *g_vs = c.vs;
        const CsEntries en = counting ? cs_entries(c, side) : CsEntries{c.ekey, c.esu, c.w, c.esu, c.w};
        if (!counting) {
            rc = sort_pairs_i32(c.tmp, c.tmp_bytes, side ? c.ki : c.ku, c.ks, c.val, c.vs, R,
                                bits_for(rows), s);
            if (rc) return rc;
        }
        const int ge = grid_for(n_pad, kBlock * 2);
        // MLP table: source row = half `side` of DX0[r]
        if (model != DAISY_NEUMF_GMF) {
            if (!counting)
                hipLaunchKernelGGL(k_nmf_entries, dim3(ge), dim3(kBlock), 0, s, g_ks, g_vs, R, n_pad, fact ? 1 : 2,
                                   fact ? 0 : side, c.ekey, c.esu, c.w);
            rc = segsum_rows(DX0, en.w_m, en.ekey, en.esu_m, n_pad, dm, sumM, c.edge_vec,
                             c.edge_item, c.edge_b, c.edge_whole, s, dx0_bf16);
            if (rc) return rc;
        }
        float *sumM_commit = (model != DAISY_NEUMF_GMF && !fact) ? sumM : (float *)nullptr;     // (fact: S_u / S_i feed the table GEMMs of csrc/neumf.hip)
        if (!pair_commit)
            launch_table_commit(side ? g.iM : g.uM, sumM_commit, side ? p.iM : p.uM, rows, dm, side ? c.ci : c.cu, side ? 3 : 1,
                                (int32_t *)nullptr, 0, 0.f, stats, reg_1, reg_2, 0, nullptr, s);
        // GMF table: source row = the materialised per-row gradient
        if (model != DAISY_NEUMF_MLP) {          // source rows: the OTHER table's, weights dpred (k_nmf_entries_gmf)
            if (!counting)
                hipLaunchKernelGGL(k_nmf_entries_gmf, dim3(ge), dim3(kBlock), 0, s, g_ks, g_vs, R, n_pad, src, side, dpred,
                                   c.ekey, c.esu, c.w);
            rc = segsum_rows(side ? p.uG : p.iG, en.w_g, en.ekey, en.esu_g, n_pad, d, sumG, c.edge_vec,
                             c.edge_item, c.edge_b, c.edge_whole, s);
            if (rc) return rc;
        }
        // (the negative item's GMF rows enter the regulariser twice, NeuMFRecommender.py:158-161)
        float *sumG_commit = (model != DAISY_NEUMF_MLP) ? sumG : (float *)nullptr;
        const float *colscale = (model != DAISY_NEUMF_MLP) ? p.Wp : (const float *)nullptr;
        if (!pair_commit)
            launch_table_commit(side ? g.iG : g.uG, sumG_commit, side ? p.iG : p.uG, rows, d, side ? c.ci : c.cu, side ? 2 : 0,
                                side ? c.cj : (int32_t *)nullptr, 4, 2.f, stats, reg_1, reg_2, 1, colscale, s);
        cside[side] = CommitSide{side ? g.iM : g.uM, sumM_commit, side ? p.iM : p.uM, dm, side ? 3 : 1,
                                 side ? g.iG : g.uG, sumG_commit, side ? p.iG : p.uG, d, side ? 2 : 0,
                                 rows, side ? c.ci : c.cu, side ? c.cj : (int32_t *)nullptr, colscale};
        DAISY_LAUNCH_CHECK();
    }
    if (pair_commit) {
        const int64_t rmax = c.U > c.I ? c.U : c.I;
        hipLaunchKernelGGL(k_nmf_table_commit_pair, dim3(grid_for(rmax, kBlock / 16), 2), dim3(kBlock), 0, s, cside[0], cside[1], stats,
                           reg_1, reg_2);
        DAISY_LAUNCH_CHECK();
    }
    return DAISY_OK;
}

void neumf_scatter_release(NeumfScatter &c) {
    c.arena.release();
    c.cs_arena.release();
}

}  // namespace daisy
