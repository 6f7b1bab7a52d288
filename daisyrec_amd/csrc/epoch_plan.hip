// The EPOCH PLAN and the static TRAIN INDEX (gfx950 / MI355X): the loader boundary of every MF / FM fit, in place of
// DataLoader(shuffle=True) over BasicDataset (daisy/utils/dataset.py:5-27 in AmazingDD/daisyRec).
//
// Every scatter of the training step is organised around OWNERSHIP instead of atomics (bpr_train.hip): an
// EPOCH PLAN (radix sorts, once per epoch) lays the epoch out batch by batch, each batch grouped by user, plus
// a per-batch list of item entries sorted by item; the item gradient is then a segmented reduction over that
// list.  That is the SORTED layout (kind 0), which every phase kernel reads.
//
// The PARTITIONED epoch plan replaces the two payload-carrying radix sorts per epoch (112 B and 80 ps per
// interaction) by two stable one-digit partitions: the training set is indexed ONCE per fit (triples in
// CSR order, item entries sorted by item: daisy_train_index), and since a stable partition of a sorted
// list by batch id leaves every batch sorted, one counting pass + one scatter pass per epoch lay the epoch
// out batch by batch.  The batch id of triple t is pos(t) / B with pos = identity, the inverse of an
// explicit permutation, or the keyed Feistel bijection of (seed, epoch) computed in registers; the stage
// slot of a sample is pos(t) - k*B, which both its sample record and its two entry records can compute
// without ever meeting.  32 B of plan per interaction.
#include <stdlib.h>
#include <string.h>

#include <atomic>

#include "epoch_plan.h"

namespace daisy {

// ids of epoch-plan builds, unique in the process (daisy_epoch_plan::build_gen)
static uint64_t next_plan_build_id() {
    static std::atomic<uint64_t> counter{0};
    return ++counter;
}

// ---------------------------------------------------------------------------
// sorted epoch plan: kernels
// ---------------------------------------------------------------------------
// order_mode: 0 identity, 1 explicit permutation (perm[p] = triple at position p), 2 Feistel
// ids outside [0,U) x [0,I) x [0,I) (point-wise rows: the third column is a label) raise *bad and are
// replaced by 0, so that no later kernel reads or writes outside the tables (daisy_epoch_plan_validate
// reports it; the reference raises IndexError in nn.Embedding, MFRecommender.py:64-65)
template <class KeyT>
__global__ void k_plan_keys(const int32_t *__restrict__ triples, const int64_t *__restrict__ perm,
                            int order_mode, FeistelKey fk, int64_t n, int64_t start, int64_t B,
                            int32_t user_base, int ubits, int64_t U, int64_t I, int pointwise,
                            int *__restrict__ bad, KeyT *__restrict__ key, uint64_t *__restrict__ val,
                            int64_t perm_limit) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n;
         e += (int64_t)gridDim.x * blockDim.x) {
        int64_t t, p;
        if (order_mode == 1) { p = e; t = perm[e]; }
        else if (order_mode == 2) { t = e; p = (int64_t)feistel_position((uint64_t)e, (uint64_t)n, fk); }
        else { t = e; p = e; }
        if (order_mode == 1 && (t < 0 || t >= perm_limit)) { atomicOr(bad, 2); t = 0; }     // (rows the entry may name)
        const int32_t *row = triples + 3 * (t + start);
        int64_t uu = (int64_t)row[0] - user_base;
        int32_t ri = row[1], rj = row[2];
        if (uu < 0 || uu >= U || ri < 0 || ri >= I || (!pointwise && (rj < 0 || rj >= I))) {
            atomicOr(bad, 1);
            uu = 0; ri = 0; rj = 0;
        }
        key[e] = (KeyT)(((uint64_t)(p / B) << ubits) | (uint64_t)uu);
        val[e] = ((uint64_t)(uint32_t)rj << 32) | (uint32_t)ri;      // (j, i)
    }
}

// from the user-grouped samples: the two item entries of every sample
template <class KeyT>
__global__ void k_plan_entries(const KeyT *__restrict__ skey, const uint64_t *__restrict__ sval,
                               int64_t n, int64_t B, int ibits, uint32_t umask, int pointwise,
                               KeyT *__restrict__ ekey, uint64_t *__restrict__ eval) {
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n;
         p += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = (uint64_t)(p / B);
        const uint32_t s = (uint32_t)(p - (int64_t)k * B);
        const uint32_t uu = (uint32_t)skey[p] & umask;
        const uint64_t ij = sval[p];
        ekey[2 * p] = (KeyT)((k << (ibits + 1)) | ((uint64_t)(uint32_t)ij << 1));
        eval[2 * p] = ((uint64_t)uu << 32) | s;
        const uint32_t jn = pointwise ? (uint32_t)ij : (uint32_t)(ij >> 32);
        ekey[2 * p + 1] = (KeyT)((k << (ibits + 1)) | ((uint64_t)jn << 1) | 1u);
        eval[2 * p + 1] = ((uint64_t)uu << 32) | (s | kNegBit);
    }
}

// 64-bit sort keys -> the 32-bit id arrays the step kernels read
__global__ void k_narrow_keys(const uint64_t *__restrict__ in, int64_t n, uint64_t mask,
                              uint32_t *__restrict__ out) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n;
         e += (int64_t)gridDim.x * blockDim.x)
        out[e] = (uint32_t)(in[e] & mask);
}

// runs of equal entry keys -> per-batch run offsets (lower bound of batch k's first key) and
// the narrowed run keys (item << 1 | neg)
template <class KeyT>
__global__ void k_run_finish(const KeyT *__restrict__ full_key, const uint32_t *__restrict__ run_total,
                             int64_t nb, int ibits1, uint32_t *__restrict__ run_key,
                             int32_t *__restrict__ run_off) {
    const int64_t R = *run_total;
    const uint64_t imask = ((uint64_t)1 << ibits1) - 1;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t m = tid; m < R; m += stride) run_key[m] = (uint32_t)((uint64_t)full_key[m] & imask);
    for (int64_t k = tid; k <= nb; k += stride) {
        const uint64_t target = (uint64_t)k << ibits1;
        int64_t lo = 0, hi = R;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((uint64_t)full_key[mid] < target) lo = mid + 1;
            else hi = mid;
        }
        run_off[k] = (int32_t)lo;
    }
}

__global__ void k_unpack_batch(BatchView v, int32_t *__restrict__ u, int32_t *__restrict__ i,
                               int32_t *__restrict__ j, int32_t *__restrict__ ent_item,
                               uint32_t *__restrict__ ent_s, int32_t *__restrict__ ent_u) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < 2 * v.B;
         e += (int64_t)gridDim.x * blockDim.x) {
        if (e < v.B) {
            u[e] = (int32_t)(v.ukey[e] & v.umask);
            i[e] = v.ij[e].x;
            j[e] = v.ij[e].y;
        }
        if (ent_item) ent_item[e] = (int32_t)((v.ekey[e] & v.imask) >> 1);
        if (ent_s) ent_s[e] = v.esu[e].x;
        if (ent_u) ent_u[e] = (int32_t)v.esu[e].y;
    }
}

// out[k] = position of triple ids[k] (a rank's rows of a multi-GPU fit)
__global__ void k_feistel_at(const int64_t *__restrict__ ids, int64_t m, int64_t n, FeistelKey fk,
                             int64_t *__restrict__ out) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = ids[e];
        out[e] = (t >= 0 && t < n) ? (int64_t)feistel_position((uint64_t)t, (uint64_t)n, fk) : -1;
    }
}

__global__ void k_feistel_perm(int64_t n, FeistelKey fk, int64_t *__restrict__ out) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n;
         e += (int64_t)gridDim.x * blockDim.x)
        out[e] = (int64_t)feistel_position((uint64_t)e, (uint64_t)n, fk);
}

// =============================================================================
// partitioned epoch plan
// =============================================================================
// DAISY_PLAN_PARK (round 5): the counting kernel of the ENTRY records parks the epoch positions its Feistel walks arrive
// at (4 B per entry, through LDS so that they leave as whole-wave stores) and the entry scatter reads them instead of
// walking again: 1.34 -> 1.22 ms per epoch at BASELINE configs[1], 2.63 -> 2.41 at 10 M x 1 M shapes.  (Not the sample
// records: their scatter is not bound by the walk - parked, it ran 348 against 361 us while its count paid 131 against 119.)  Round 4 had taken this out ("a tie"): then the
// scatter wrote 2.1 x its records in partial lines and was bound by that; with array-of-structures records every plan
// kernel runs at 84-100 % of the VALU issue rate (profiles/r05_pmc_plan.txt: 651 M wave instructions x 4 cycles over
// 1024 SIMDs = 1.06 of the 1.27 ms) while the build moves 3.3 GB in 1.27 ms - the memory system is the idle side now.
#ifndef DAISY_PLAN_PARK
#define DAISY_PLAN_PARK 1
#endif
constexpr int kPartThreads = 256;
constexpr int kPartK = 8;                              // records per thread per sub-tile: samples (16-byte records)
constexpr int kPartKE = 8;                             //   entries (8-byte records; 16 per thread measured 1.56 against
                                                       //   1.30 ms per epoch at BASELINE configs[1]: two workgroups per CU
                                                       //   less, and every lane walks twice as many positions in a row)
constexpr int kPartSub = kPartThreads * kPartK;        // 2048 records: the counting kernels' staging unit
constexpr int kPartMaxTiles = 16384;                   // most tiles (workgroups) of a partition
constexpr int kPartWaves = kPartThreads / kWave;

struct PosFn {            // position of triple t in the epoch order
    int mode;             // daisy_order_mode
    FeistelKey fk;
    const uint32_t *inv;  // DAISY_ORDER_PERM: inv[t] = p with perm[p] = t
    const uint32_t *orig; // CSR row -> row of the caller's triple array (NULL: the array was in CSR order)
    uint64_t n;
};
__device__ __forceinline__ uint32_t pos_of(const PosFn &f, uint32_t t) {
    if (f.orig) t = f.orig[t];
    if (f.mode == DAISY_ORDER_FEISTEL) return (uint32_t)feistel_position((uint64_t)t, f.n, f.fk);
    if (f.mode == DAISY_ORDER_PERM) return f.inv[t];
    return t;
}
struct BatchDiv { uint32_t B, M0; int shift; };   // batch id = p / B without a hardware divide
static BatchDiv make_batch_div(int64_t B) {
    BatchDiv bd;
    bd.B = (uint32_t)B;
    bd.M0 = (B >= 2) ? (uint32_t)(((uint64_t)1 << 32) / (uint64_t)B) : 0u;
    bd.shift = -1;
    if ((B & (B - 1)) == 0) { bd.shift = 0; while (((int64_t)1 << bd.shift) < B) ++bd.shift; }
    return bd;
}
__device__ __forceinline__ uint32_t batch_of(uint32_t p, const BatchDiv &bd) {
    if (bd.shift >= 0) return p >> bd.shift;          // power-of-two batch (uniform branch)
    uint32_t q = __umulhi(p, bd.M0);        // floor(p*floor(2^32/B)/2^32) in {q_true-1, q_true}
    uint32_t r = p - q * bd.B;
    while (r >= bd.B) { r -= bd.B; ++q; }
    return q;
}

// Records of the partitioned plan (array of structures: a bucket piece of a sub-tile leaves as ONE contiguous run of
// 16-byte / 8-byte records - round 3's three separate arrays left as ~85-record pieces of 340 / 680 / 340 B, and the
// counters showed the scatter writing 2.1x its records in partial lines):
//   sample record  uint4 {user, pos item, neg item (or label), epoch position}
//   entry record   uint2 {item << 1 | slot, epoch position of its sample}
struct PartSrc {
    const int32_t *triples; int32_t user_base;          // samples, static source (CSR-ordered triples)
    const uint32_t *ent_t;                              // entries, static source: triple index | slot << 31
    const uint32_t *ent_key;                            //                         item << 1 | slot
    const uint4 *srec;                                  // samples, record source (LSD pass >= 1)
    const uint2 *erec;                                  // entries, record source
    uint32_t *park;                                     // the kind's parked epoch positions (device shuffle, first pass)
};
struct PartDst { uint4 *srec; uint2 *erec; };

// lanes of this wave that hold the same digit (the AMD counterpart of match.any: one ballot per digit bit)
__device__ __forceinline__ uint64_t match_digit(uint32_t dgt, bool valid, int nbits) {
    uint64_t peers = __ballot(valid);
    for (int b = 0; b < nbits; ++b) {
        const bool bit = (dgt >> b) & 1u;
        const uint64_t m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    return peers;
}

// Digit histogram of every tile.  KIND 0: samples from the static source   1: entries from the static source (their
// epoch positions are computed here and again by the scatter pass - round 3 parked them in memory for it: 12 B per
// record of traffic for ALU work that hides under the scatter's memory time; measured a tie to slightly faster,
// profiles/r04_plan_variants.txt "variant 3")   2 / 3: sample / entry records of a previous LSD pass.
template <int KIND>
__global__ __launch_bounds__(kPartThreads) void k_part_count(PartSrc src, PosFn pf, BatchDiv bd, int64_t n,
                                                             int shift, int nbits, int ndig, int64_t tile_elems,
                                                             int64_t ntiles, uint32_t *__restrict__ counts) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t lds_t[KIND == 1 ? kPartSub : 1];
    // the positions of a sub-tile wait here for ONE coalesced store per thread and round: stored from inside the walk -
    // a few lanes per trip - they made 440 us of count<entries>'s 262 (profiles/r05_notes.txt)
    __shared__ uint32_t lds_p[(DAISY_PLAN_PARK && KIND == 1) ? kPartSub : 1];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * tile_elems;
    const int64_t hi = (lo + tile_elems < n) ? lo + tile_elems : n;
    if (KIND < 2 && pf.mode == DAISY_ORDER_FEISTEL) {
        // Cycle walking inside a lock-step wave costs the MAXIMUM walk length of its 64 lanes per element
        // (~3.5 network passes instead of the 1.34 average at n = 0.75 * 2^2h).  So every lane owns a strip of
        // elements and steps through it at its own pace: each trip of the loop is one useful network pass for
        // every lane, and the lanes only wait for each other at the end of the strip.
        const uint32_t nn = (uint32_t)pf.n;
        for (int64_t sub = lo; sub < hi; sub += kPartSub) {
            if constexpr (KIND == 1) {
                __syncthreads();
#pragma unroll
                for (int k = 0; k < kPartK; ++k) {
                    const int64_t e = sub + k * kPartThreads + threadIdx.x;
                    lds_t[k * kPartThreads + threadIdx.x] = (e < hi) ? (src.ent_t[e] & ~kNegBit) : 0u;
                }
                __syncthreads();
            }
            int j = 0;
            int64_t e = sub + threadIdx.x;
            bool active = e < hi;
            auto first = [&]() -> uint32_t {
                uint32_t t;
                if constexpr (KIND == 1) t = lds_t[j * kPartThreads + threadIdx.x];
                else t = (uint32_t)e;
                return pf.orig ? pf.orig[t] : t;
            };
            uint32_t x = active ? first() : 0u;
            while (active) {
                x = feistel_once(x, pf.fk);
                if (x < nn) {
                    atomicAdd(&hist[(batch_of(x, bd) >> shift) & 255u], 1u);
                    if constexpr (DAISY_PLAN_PARK && KIND == 1) lds_p[j * kPartThreads + threadIdx.x] = x;
                    ++j;
                    e += kPartThreads;
                    active = (j < kPartK) && (e < hi);
                    if (active) x = first();
                }
            }
            if constexpr (DAISY_PLAN_PARK && KIND == 1) {
                // (each thread reads back what it wrote: no barrier; element sub + k * 256 + thread: coalesced)
#pragma unroll
                for (int k = 0; k < kPartK; ++k) {
                    const int64_t ek = sub + k * kPartThreads + threadIdx.x;
                    if (ek < hi) src.park[ek] = lds_p[k * kPartThreads + threadIdx.x];
                }
            }
        }
    } else {
        const uint64_t lt_mask = ((uint64_t)1 << (threadIdx.x % kWave)) - 1;
        for (int64_t base = lo; base < hi; base += kPartThreads) {
            const int64_t e = base + threadIdx.x;
            const bool valid = e < hi;
            uint32_t p = 0;
            if (valid) {
                if constexpr (KIND == 0) p = pos_of(pf, (uint32_t)e);
                else if constexpr (KIND == 1) p = pos_of(pf, src.ent_t[e] & ~kNegBit);
                else if constexpr (KIND == 2) p = src.srec[e].w;
                else p = src.erec[e].y;
            }
            const uint32_t dgt = (batch_of(p, bd) >> shift) & 255u;
            const uint64_t peers = match_digit(dgt, valid, nbits);          // one LDS atomic per digit per wave
            if (valid && (peers & lt_mask) == 0) atomicAdd(&hist[dgt], (uint32_t)__popcll(peers));
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < ndig) counts[(int64_t)threadIdx.x * ntiles + blockIdx.x] = hist[threadIdx.x];
}

// Stable scatter of one LSD digit.  A tile is cut into sub-tiles of 256 * K records; a wave takes 64 * K consecutive
// records of the sub-tile in K rounds of 64 (coalesced reads, and the round order = the record order, so ranks are
// stable), the sub-tile is sorted by digit in LDS and every bucket leaves as one contiguous piece of whole records.
// STATIC: the records are formed from the static index and their epoch positions are computed here - every lane walks
// the Feistel network over its own K records (k_part_count's strip walk) into LDS while the other workgroups of the CU
// are in their memory phases.
template <bool SAMPLES, bool STATIC, int K>
__global__ __launch_bounds__(kPartThreads) void k_part_scatter(PartSrc src, PosFn pf, BatchDiv bd, int64_t n,
                                                               int shift, int nbits, int ndig,
                                                               int64_t tile_elems, int64_t ntiles,
                                                               const uint32_t *__restrict__ offsets, uint32_t off_base,
                                                               PartDst dst) {
    constexpr int SUB = kPartThreads * K;
    // the sorted records; before that (STATIC) the sub-tile's epoch positions, 4 B per record, read back by the thread
    // that wrote them and dead by the time the first record is stored (two barriers in between)
    __shared__ __attribute__((aligned(16))) uint32_t recw[SUB * (SAMPLES ? 4 : 2)];
    __shared__ uint8_t sdig[SUB];
    __shared__ uint32_t wcnt[kPartWaves][256];
    __shared__ uint32_t tstart[256], goff[256], tot[256];
    __shared__ uint32_t wsum[kPartWaves];
    uint4 *rec4 = reinterpret_cast<uint4 *>(recw);
    uint2 *rec2 = reinterpret_cast<uint2 *>(recw);
    uint32_t *lp = recw;

    const int tid = threadIdx.x, wave = tid / kWave, wl = tid % kWave;
    const uint64_t lt_mask = ((uint64_t)1 << wl) - 1;
    goff[tid] = (tid < ndig) ? offsets[(int64_t)tid * ntiles + blockIdx.x] - off_base : 0u;
    const int64_t lo = (int64_t)blockIdx.x * tile_elems;
    const int64_t hi = (lo + tile_elems < n) ? lo + tile_elems : n;

    for (int64_t sub = lo; sub < hi; sub += SUB) {
#pragma unroll
        for (int w = 0; w < kPartWaves; ++w) wcnt[w][tid] = 0;
        uint32_t r_a[K], r_b[SAMPLES ? K : 1], r_c[SAMPLES ? K : 1], r_p[K], r_rank[K], r_dig[K];
        const int64_t wbase = sub + (int64_t)wave * (kWave * K);
        // ---- the records of this thread (round r: record wbase + r*64 + wl); all loads are issued before the walk
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const int64_t e = wbase + r * kWave + wl;
            const int64_t ec = (e < hi) ? e : hi - 1;
            if constexpr (!STATIC) {
                if constexpr (SAMPLES) {
                    const uint4 q = src.srec[ec];
                    r_a[r] = q.x; r_b[r] = q.y; r_c[r] = q.z; r_p[r] = q.w;
                } else {
                    const uint2 q = src.erec[ec];
                    r_a[r] = q.x; r_p[r] = q.y;
                }
            } else if constexpr (SAMPLES) {
                const int32_t *row = src.triples + 3 * ec;
                r_a[r] = (uint32_t)(row[0] - src.user_base);
                r_b[r] = (uint32_t)row[1];
                r_c[r] = (uint32_t)row[2];
                r_p[r] = (uint32_t)ec;                      // (the triple whose position is wanted)
            } else {
                r_a[r] = src.ent_key[ec];
                r_p[r] = src.ent_t[ec] & ~kNegBit;
            }
        }
        if constexpr (STATIC) {
            // slot of the record this thread holds in round r: wave*64*K + r*64 + wl
            const int xw = wave * (kWave * K) + wl;
            if (DAISY_PLAN_PARK && !SAMPLES && pf.mode == DAISY_ORDER_FEISTEL) {
#pragma unroll
                for (int r = 0; r < K; ++r) {              // parked by k_part_count: no second walk
                    const int64_t e = wbase + r * kWave + wl;
                    r_p[r] = src.park[(e < hi) ? e : hi - 1];
                }
            } else if (pf.mode == DAISY_ORDER_FEISTEL) {
                const uint32_t nn = (uint32_t)pf.n;
#pragma unroll
                for (int r = 0; r < K; ++r) lp[xw + r * kWave] = pf.orig ? pf.orig[r_p[r]] : r_p[r];
                int r = 0;
                bool active = wbase + wl < hi;
                uint32_t v = active ? lp[xw] : 0u;
                while (active) {
                    v = feistel_once(v, pf.fk);
                    if (v < nn) {
                        lp[xw + r * kWave] = v;
                        ++r;
                        active = (r < K) && (wbase + r * kWave + wl < hi);
                        if (active) v = lp[xw + r * kWave];
                    }
                }
#pragma unroll
                for (int r = 0; r < K; ++r) r_p[r] = lp[xw + r * kWave];
            } else {
#pragma unroll
                for (int r = 0; r < K; ++r) r_p[r] = pos_of(pf, r_p[r]);
            }
        }
        __syncthreads();              // (wcnt is zero; nobody is still reading the previous sub-tile's records)
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const bool valid = wbase + r * kWave + wl < hi;
            const uint32_t dgt = (batch_of(r_p[r], bd) >> shift) & 255u;
            const uint64_t peers = match_digit(dgt, valid, nbits);
            const uint32_t base = wcnt[wave][dgt];                  // all lanes read ...
            const uint32_t rank = (uint32_t)__popcll(peers & lt_mask);
            if (valid && rank == 0) wcnt[wave][dgt] = base + (uint32_t)__popcll(peers);   // ... then one lane per digit writes
            r_rank[r] = base + rank;
            r_dig[r] = valid ? dgt : 0xFFFFFFFFu;
        }
        __syncthreads();
        // digit totals of the sub-tile, their exclusive scan, and the waves' offsets inside each digit
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < kPartWaves; ++w) { const uint32_t c = wcnt[w][tid]; wcnt[w][tid] = t; t += c; }
        tot[tid] = t;
        uint32_t inc = t;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const uint32_t up = __shfl_up(inc, off, kWave);
            if (wl >= off) inc += up;
        }
        if (wl == kWave - 1) wsum[wave] = inc;
        __syncthreads();
        uint32_t wprefix = 0;
#pragma unroll
        for (int w = 0; w < kPartWaves; ++w) if (w < wave) wprefix += wsum[w];
        tstart[tid] = wprefix + inc - t;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < K; ++r) {
            if (r_dig[r] != 0xFFFFFFFFu) {
                const uint32_t x = tstart[r_dig[r]] + wcnt[wave][r_dig[r]] + r_rank[r];
                if constexpr (SAMPLES) rec4[x] = make_uint4(r_a[r], r_b[r], r_c[r], r_p[r]);
                else rec2[x] = make_uint2(r_a[r], r_p[r]);
                sdig[x] = (uint8_t)r_dig[r];
            }
        }
        __syncthreads();
        const int cnt = (int)((hi - sub < SUB) ? (hi - sub) : SUB);
        for (int x = tid; x < cnt; x += kPartThreads) {
            const uint32_t dg = sdig[x];
            const int64_t o = (int64_t)goff[dg] + (x - tstart[dg]);
            if constexpr (SAMPLES) dst.srec[o] = rec4[x];
            else dst.erec[o] = rec2[x];
        }
        __syncthreads();
        goff[tid] += tot[tid];
    }
}

// inv[perm[p]] = p  (DAISY_ORDER_PERM: perm[p] = triple served at position p)
__global__ void k_invert_perm(const int64_t *__restrict__ perm, int64_t n, uint32_t *__restrict__ inv) {
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = perm[p];
        if (t >= 0 && t < n) inv[t] = (uint32_t)p;
    }
}

// positions handed in by the caller (daisy_epoch_plan_build_positions): inv[t] = pos[t]; bad |= 2 outside [0, n_total)
__global__ void k_positions_u32(const int64_t *__restrict__ pos, int64_t n, int64_t n_total, uint32_t *__restrict__ inv,
                                int *__restrict__ bad) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = pos[t];
        const bool ok = p >= 0 && p < n_total;
        if (!ok) atomicOr(bad, 2);
        inv[t] = ok ? (uint32_t)p : 0u;
    }
}

// off[k] = first record of batch k in the partitioned sample records (their batch ids never decrease)
__global__ void k_batch_offsets(const uint4 *__restrict__ srec, int64_t n, BatchDiv bd, int64_t nb,
                                int64_t *__restrict__ off) {
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k <= nb; k += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = n;                       // first index whose batch id >= k
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)batch_of(srec[mid].w, bd) < k) lo = mid + 1; else hi = mid;
        }
        off[k] = lo;
    }
}

// ---- static index ---------------------------------------------------------------------------------------
// bad[0] |= 1 when a (user - user_base, item, item) lies outside [0,U) x [0,I) x [0,I)
// pointwise: rows are (user, item, label) - one entry per row, the third column is not an id
__global__ void k_index_entries(const int32_t *__restrict__ triples, int64_t n, int32_t user_base, int64_t U,
                                int64_t I, uint32_t *__restrict__ key, uint32_t *__restrict__ val,
                                uint32_t *__restrict__ ukey, uint32_t *__restrict__ uval, int *__restrict__ bad,
                                int pointwise) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int32_t *row = triples + 3 * t;
        const int64_t u = (int64_t)row[0] - user_base, i = row[1], j = row[2];
        const bool ok = u >= 0 && u < U && i >= 0 && i < I && (pointwise || (j >= 0 && j < I));
        if (!ok) atomicOr(bad, 1);
        if (key && pointwise) {
            key[t] = ok ? ((uint32_t)i << 1) : 0u;
            val[t] = (uint32_t)t;
        } else if (key) {
            key[2 * t] = ok ? ((uint32_t)i << 1) : 0u;
            val[2 * t] = (uint32_t)t;
            key[2 * t + 1] = ok ? (((uint32_t)j << 1) | 1u) : 1u;
            val[2 * t + 1] = (uint32_t)t | kNegBit;
        }
        if (ukey) { ukey[t] = ok ? (uint32_t)u : 0u; uval[t] = (uint32_t)t; }
    }
}

// entries per item (once per fit): the longest segment an item pass can meet decides how its edge chains are reduced.
// The entries are sorted by item: a segment's first and last entry write their (1-based) places - plain stores, one per
// item (an atomic histogram of the sorted list put a thousand consecutive adds on every address: 8.6 ms at 100 M entries).
__global__ void k_item_bounds(const uint32_t *__restrict__ ent_key, int64_t n_ent, uint32_t *__restrict__ first,
                              uint32_t *__restrict__ last) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n_ent; e += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t it = ent_key[e] >> 1;
        if (e == 0 || (ent_key[e - 1] >> 1) != it) first[it] = (uint32_t)e + 1u;
        if (e == n_ent - 1 || (ent_key[e + 1] >> 1) != it) last[it] = (uint32_t)e + 1u;
    }
}
__global__ void k_item_max_len(const uint32_t *__restrict__ first, const uint32_t *__restrict__ last, int64_t n,
                               uint32_t *__restrict__ out) {
    uint32_t m = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t len = last[i] ? last[i] - first[i] + 1u : 0u;
        m = len > m ? len : m;
    }
    atomicMax(out, m);
}

__global__ void k_gather_triples(const int32_t *__restrict__ triples, const uint32_t *__restrict__ order, int64_t n,
                                 int32_t *__restrict__ out) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t *row = triples + 3 * (int64_t)order[e];
        out[3 * e] = row[0]; out[3 * e + 1] = row[1]; out[3 * e + 2] = row[2];
    }
}

__global__ void k_read_partitioned(StreamView v, int32_t *__restrict__ u, int32_t *__restrict__ i,
                                   int32_t *__restrict__ j, int32_t *__restrict__ ent_item,
                                   uint32_t *__restrict__ ent_s, int32_t *__restrict__ ent_u) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < v.E; e += (int64_t)gridDim.x * blockDim.x) {
        if (e < v.B) {
            const uint4 r = sv_sample(v, e);
            u[e] = (int32_t)r.x;
            i[e] = (int32_t)r.y;
            j[e] = (int32_t)r.z;
        }
        const uint32_t k = sv_key(v, e);
        if (ent_item) ent_item[e] = (int32_t)(k >> 1);
        if (ent_s) ent_s[e] = ((v.e_pos[e * v.e_stride] & ~kNegBit) - v.pos_base) | ((k & 1u) ? kNegBit : 0u);
        if (ent_u) ent_u[e] = -1;          // this layout does not carry the user with the entry
    }
}

// ---------------------------------------------------------------------------
// plan construction (host side)
// ---------------------------------------------------------------------------
int plan_alloc(daisy_epoch_plan **out, int64_t max_triples, int64_t U, int64_t I) {
    daisy_epoch_plan *p = new daisy_epoch_plan();      // (all zero: no device memory yet, each layout allocates at its first build)
    p->max_triples = max_triples; p->U = U; p->I = I;
    *out = p;
    return DAISY_OK;
}

// buffers of the sorted layout (kind 0)
static int plan_need_sorted(daisy_epoch_plan *p) {
    if (p->arena.bytes()) return DAISY_OK;
    const int64_t max_triples = p->max_triples;
    const size_t n2 = 2 * (size_t)max_triples;
    const size_t ta = sort_pairs_u32_u64_temp_bytes(n2), tb = sort_pairs_u64_u64_temp_bytes(n2);
    const size_t tc = rle_u32_temp_bytes(n2), td = rle_u64_temp_bytes(n2);
    p->temp_bytes = ta > tb ? ta : tb;
    if (tc > p->temp_bytes) p->temp_bytes = tc;
    if (td > p->temp_bytes) p->temp_bytes = td;
    DeviceArena &a = p->arena;
    a.add(&p->k32[0], n2 * 4); a.add(&p->k32[1], n2 * 4);
    a.add(&p->v64[0], n2 * 8); a.add(&p->v64[1], n2 * 8);
    a.add(&p->ukey, (size_t)max_triples * 4);   // sorted sample keys survive the entry sort
    a.add(&p->uval, (size_t)max_triples * 8);
    a.add(&p->run_key, n2 * 4); a.add(&p->run_cnt, n2 * 4); a.add(&p->run_off, ((size_t)max_triples + 2) * 4);
    a.add(&p->run_total, 256);
    a.add(&p->temp, p->temp_bytes);
    if (int rc = a.alloc("epoch_plan_build")) {
        a.release();
        return rc;
    }
    p->bad = (int *)((char *)p->run_total + 64);       // (k64: allocated on demand - rare: > 32 key bits)
    return DAISY_OK;
}

// a plan that held a rank's share of the epoch (daisy_epoch_plan_build_positions) forgets its batch offsets
static void plan_drop_offsets(daisy_epoch_plan *p) {
    free(p->h_off);
    if (p->d_off) (void)hipFree(p->d_off);
    p->h_off = nullptr; p->d_off = nullptr; p->h_off_cap = 0;
}

size_t plan_bytes(const daisy_epoch_plan *p) { return p->arena.bytes() + p->part[0].bytes() + p->part[1].bytes(); }

int plan_free(daisy_epoch_plan *p) {
    const hipError_t e = p->arena.release() ? hipSuccess : hipGetLastError();
    for (int k = 0; k < 2; ++k) {
        if (p->k64[k]) (void)hipFree(p->k64[k]);
        (void)p->part[k].release();
    }
    plan_drop_offsets(p);
    delete p;
    if (e != hipSuccess) {
        set_error("epoch_plan_destroy: hipFree failed: %s", hipGetErrorString(e));
        return DAISY_ERR_HIP;
    }
    return DAISY_OK;
}

static int plan_need_k64(daisy_epoch_plan *p) {
    for (int k = 0; k < 2; ++k) {
        if (!p->k64[k]) {
            hipError_t e = hipMalloc((void **)&p->k64[k], 2 * (size_t)p->max_triples * 8);
            if (e != hipSuccess) {
                set_error("epoch_plan_build: hipMalloc of 64-bit key buffers failed: %s", hipGetErrorString(e));
                return DAISY_ERR_HIP;
            }
        }
    }
    return DAISY_OK;
}

// flags: DAISY_PLAN_TRIPLES_USER_SORTED -> the samples only need a stable partition by batch
// perm_limit: rows of `triples` a permutation entry may name (n for a permutation of the n rows; the whole array when the
// entries SELECT n of its rows: daisy_bpr_set_batch_from_triples - whose range check compared against n until round 4, so
// that a selection naming a row >= its own length was refused)
int plan_build(daisy_epoch_plan *p, const int32_t *triples, int64_t n, int64_t start,
               const int64_t *perm, int order_mode, uint64_t seed, uint64_t epoch,
               int64_t batch_size, int32_t user_base, int32_t flags, hipStream_t s, int64_t perm_limit) {
    if (perm_limit < 0) perm_limit = n;
    const int ubits = bits_for(p->U), ibits = bits_for(p->I);
    const int64_t nb = (n + batch_size - 1) / batch_size;
    const int bbits = (nb > 1) ? bits_for(nb) : 0;
    const uint32_t umask = (uint32_t)(((uint64_t)1 << ubits) - 1);
    const int ibits1 = ibits + 1;                    // item << 1 | negative-slot bit
    const uint32_t imask = (uint32_t)(((uint64_t)1 << ibits1) - 1);
    const bool wide = (ubits + bbits > 32) || (ibits1 + bbits > 32);
    const bool presorted = (flags & DAISY_PLAN_TRIPLES_USER_SORTED) && order_mode != DAISY_ORDER_PERM;
    const int pointwise = (flags & DAISY_PLAN_POINTWISE) ? 1 : 0;
    int rc = plan_need_sorted(p);
    if (rc) return rc;
    const int s_begin = presorted ? ubits : 0;      // user bits ride along unsorted
    FeistelKey fk = make_feistel_key((uint64_t)n, seed, epoch);
    const int g1 = grid_for(n, kBlock), g2 = grid_for(2 * n, kBlock);
    DAISY_HIP(hipMemsetAsync(p->bad, 0, sizeof(int), s));
    if (!wide) {
        hipLaunchKernelGGL((k_plan_keys<uint32_t>), dim3(g1), dim3(kBlock), 0, s, triples, perm,
                           order_mode, fk, n, start, batch_size, user_base, ubits, p->U, p->I, pointwise, p->bad,
                           p->k32[0], p->v64[0], perm_limit);
        DAISY_LAUNCH_CHECK();
        if (ubits + bbits > s_begin) {
            rc = sort_pairs_u32_u64(p->temp, p->temp_bytes, p->k32[0], p->ukey, p->v64[0], p->uval, n,
                                    s_begin, ubits + bbits, s);
            if (rc) return rc;
        } else {   // one batch of user-sorted triples: already in plan order
            DAISY_HIP(hipMemcpyAsync(p->ukey, p->k32[0], n * 4, hipMemcpyDeviceToDevice, s));
            DAISY_HIP(hipMemcpyAsync(p->uval, p->v64[0], n * 8, hipMemcpyDeviceToDevice, s));
        }
        hipLaunchKernelGGL((k_plan_entries<uint32_t>), dim3(g1), dim3(kBlock), 0, s, p->ukey, p->uval,
                           n, batch_size, ibits, umask, pointwise, p->k32[0], p->v64[0]);
        DAISY_LAUNCH_CHECK();
        rc = sort_pairs_u32_u64(p->temp, p->temp_bytes, p->k32[0], p->k32[1], p->v64[0], p->v64[1], 2 * n,
                                0, ibits1 + bbits, s);
        if (rc) return rc;
        // runs of equal (batch, item, slot) keys: the distinct items of every batch + their counts
        rc = rle_u32(p->temp, p->temp_bytes, p->k32[1], 2 * n, p->k32[0], p->run_cnt, p->run_total, s);
        if (rc) return rc;
        hipLaunchKernelGGL((k_run_finish<uint32_t>), dim3(g2), dim3(kBlock), 0, s, p->k32[0], p->run_total,
                           nb, ibits1, p->run_key, p->run_off);
        DAISY_LAUNCH_CHECK();
        p->umask = umask;
        p->imask = imask;
    } else {
        if ((rc = plan_need_k64(p))) return rc;
        hipLaunchKernelGGL((k_plan_keys<uint64_t>), dim3(g1), dim3(kBlock), 0, s, triples, perm,
                           order_mode, fk, n, start, batch_size, user_base, ubits, p->U, p->I, pointwise, p->bad,
                           p->k64[0], p->v64[0], perm_limit);
        DAISY_LAUNCH_CHECK();
        rc = sort_pairs_u64_u64(p->temp, p->temp_bytes, p->k64[0], p->k64[1], p->v64[0], p->uval, n,
                                s_begin, ubits + bbits, s);
        if (rc) return rc;
        hipLaunchKernelGGL(k_narrow_keys, dim3(g1), dim3(kBlock), 0, s, p->k64[1], n, (uint64_t)umask,
                           p->ukey);
        DAISY_LAUNCH_CHECK();
        hipLaunchKernelGGL((k_plan_entries<uint64_t>), dim3(g1), dim3(kBlock), 0, s, p->k64[1], p->uval,
                           n, batch_size, ibits, 0xFFFFFFFFu & umask, pointwise, p->k64[0], p->v64[0]);
        DAISY_LAUNCH_CHECK();
        rc = sort_pairs_u64_u64(p->temp, p->temp_bytes, p->k64[0], p->k64[1], p->v64[0], p->v64[1], 2 * n,
                                0, ibits1 + bbits, s);
        if (rc) return rc;
        rc = rle_u64(p->temp, p->temp_bytes, p->k64[1], 2 * n, p->k64[0], p->run_cnt, p->run_total, s);
        if (rc) return rc;
        hipLaunchKernelGGL((k_run_finish<uint64_t>), dim3(g2), dim3(kBlock), 0, s, p->k64[0], p->run_total,
                           nb, ibits1, p->run_key, p->run_off);
        DAISY_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_narrow_keys, dim3(g2), dim3(kBlock), 0, s, p->k64[1], 2 * n, (uint64_t)imask,
                           p->k32[1]);
        DAISY_LAUNCH_CHECK();
        p->umask = 0xFFFFFFFFu;
        p->imask = 0xFFFFFFFFu;
    }
    p->ekey = p->k32[1];
    p->eval = p->v64[1];
    plan_drop_offsets(p);
    p->n = n; p->batch_size = batch_size; p->num_batches = nb; p->built = true;
    p->build_gen = next_plan_build_id();
    p->pointwise = pointwise;
    p->kind = 0;
    return DAISY_OK;
}

BatchView plan_view(const daisy_epoch_plan *p, int64_t k) {
    const int64_t lo = k * p->batch_size;
    BatchView v;
    v.B = (p->n - lo < p->batch_size) ? (p->n - lo) : p->batch_size;
    v.ukey = p->ukey + lo;
    v.ij = reinterpret_cast<const int2 *>(p->uval + lo);
    v.ekey = p->ekey + 2 * lo;
    v.esu = reinterpret_cast<const uint2 *>(p->eval + 2 * lo);
    v.run_key = p->run_key;
    v.run_cnt = p->run_cnt;
    v.run_off = p->run_off + k;
    v.umask = p->umask;
    v.imask = p->imask;
    v.pointwise = p->pointwise;
    v.bu = v.bi = v.b0 = v.g_bu = v.g_bi = v.g_b0 = nullptr;
    v.halt = nullptr;
    return v;
}

// the same batch as the staged step reads it (stage slot = grouped sample position)
StreamView stream_view_of(const BatchView &v) {
    StreamView sv;
    sv.s_rec = nullptr; sv.s_user = v.ukey; sv.s_ij = v.ij;
    sv.e_key = v.ekey; sv.e_kstride = 1; sv.e_pos = reinterpret_cast<const uint32_t *>(v.esu); sv.e_stride = 2;
    sv.umask = v.umask; sv.imask = v.imask; sv.pos_base = 0;
    sv.B = v.B; sv.E = 2 * v.B;
    sv.halt = nullptr;
    sv.pointwise = v.pointwise;
    sv.p_stream = 0;
    return sv;
}

StreamView plan_stream_view(const daisy_epoch_plan *p, int64_t k) {
    int64_t lo = k * p->batch_size;
    const int c = p->p_cur;
    StreamView v;
    v.B = (p->n - lo < p->batch_size) ? (p->n - lo) : p->batch_size;
    const uint32_t pos_base = (uint32_t)lo;           // stage slot = epoch position - k*B in both layouts
    if (p->h_off) { lo = p->h_off[k]; v.B = p->h_off[k + 1] - lo; }      // a rank's share of the epoch
    const int64_t epl = p->pointwise ? 1 : 2;          // entries per sample (point-wise rows have no negative item)
    v.E = epl * v.B;
    v.s_rec = p->p_srec[c] + lo;
    v.s_user = nullptr; v.s_ij = nullptr;
    v.e_key = reinterpret_cast<const uint32_t *>(p->p_erec[c] + epl * lo);      // record {key, pos}: both at stride 2
    v.e_pos = v.e_key + 1;
    v.e_kstride = 2;
    v.e_stride = 2;
    v.umask = v.imask = 0xFFFFFFFFu;
    v.pos_base = pos_base;
    v.halt = nullptr;
    v.pointwise = p->pointwise;
    v.p_stream = 0;
    return v;
}

static int plan_read_batch_partitioned(const daisy_epoch_plan *plan, int64_t k, int32_t *u, int32_t *i, int32_t *j,
                                       int32_t *ent_item, uint32_t *ent_s, int32_t *ent_u, int64_t *B_out_host,
                                       hipStream_t s) {
    const StreamView v = plan_stream_view(plan, k);
    hipLaunchKernelGGL(k_read_partitioned, dim3(grid_for(v.E, kBlock)), dim3(kBlock), 0, s, v, u, i, j, ent_item,
                       ent_s, ent_u);
    DAISY_LAUNCH_CHECK();
    if (B_out_host) *B_out_host = v.B;
    return DAISY_OK;
}

// record set x of the partitioned layout lives in one allocation: sample records [n] x 16 B, entry records [2n] x 8 B;
// set 0 also carries what every build needs: the tile counts, the scan scratch, the inverse permutation, the park
static int plan_need_partitioned(daisy_epoch_plan *p, int set) {
    DeviceArena &a = p->part[set];
    if (a.bytes()) return DAISY_OK;
    const size_t n = (size_t)p->max_triples;
    size_t cnt_elems = 0;
    a.add(&p->p_srec[set], n * 16); a.add(&p->p_erec[set], n * 16);
    if (set == 0) {
        const int64_t max_tiles = (2 * (int64_t)n + kPartSub - 1) / kPartSub;
        const int64_t tiles = max_tiles < kPartMaxTiles ? max_tiles : kPartMaxTiles + 1;
        cnt_elems = (size_t)256 * (size_t)(tiles + 1);
        p->p_scan_bytes = exclusive_scan_u32_temp_bytes((int64_t)cnt_elems);
        a.add(&p->p_counts, cnt_elems * 4 * 2);   // counts, then their exclusive scan
        a.add(&p->p_scan, p->p_scan_bytes);
        a.add(&p->p_inv, n * 4);
        if (DAISY_PLAN_PARK) a.add(&p->p_park, n * 8);
    }
    if (int rc = a.alloc("epoch_plan_build_indexed")) {
        a.release();
        return rc;
    }
    if (set == 0) p->p_offsets = p->p_counts + cnt_elems;
    return DAISY_OK;
}

// tiles (workgroups) of a partition over n records whose sub-tiles hold `sub` records: at most kPartMaxTiles (the count
// buffers hold that many; fewer, longer tiles measured slower - profiles/r04_plan_variants.txt)
static void part_tiling(int64_t n, int64_t sub, int64_t &tile_elems, int64_t &ntiles) {
    // DAISY_PART_TILES: fewer tiles than the buffers hold (read per build).  Tiles of several sub-tiles otherwise need
    // more than 67 M records: the tests use it to walk that loop on small plans
    const char *env = getenv("DAISY_PART_TILES");
    int64_t cap = env ? atoll(env) : kPartMaxTiles;
    cap = cap < 1 ? 1 : (cap > kPartMaxTiles ? kPartMaxTiles : cap);
    int64_t subs = (n + sub * cap - 1) / (sub * cap);
    if (subs < 1) subs = 1;
    tile_elems = subs * sub;
    ntiles = (n + tile_elems - 1) / tile_elems;
}

// n_total == 0: the index holds the whole epoch (n rows, positions 0..n-1 from `order_mode`).  n_total > 0: it holds
// a subset and `perm` is not a permutation but the epoch POSITION of every caller row, in [0, n_total): batch k is
// made of the held rows with position in [k*B, (k+1)*B), so the batches have different sizes (h_off).
static int plan_build_partitioned(daisy_epoch_plan *p, const daisy_train_index *ix, const int64_t *perm,
                                  int order_mode, uint64_t seed, uint64_t epoch, int64_t batch_size,
                                  int64_t n_total, hipStream_t s) {
    const int64_t n = ix->n;
    const bool subset = n_total > 0;
    const int64_t nb = ((subset ? n_total : n) + batch_size - 1) / batch_size;
    const int bbits = (nb > 1) ? bits_for(nb) : 1;
    const int passes = (bbits + 7) / 8;
    int rc = plan_need_partitioned(p, 0);
    if (rc) return rc;
    if (passes > 1 && (rc = plan_need_partitioned(p, 1))) return rc;
    PosFn pf;
    pf.mode = order_mode;
    pf.fk = make_feistel_key((uint64_t)n, seed, epoch);
    pf.inv = p->p_inv;
    pf.orig = ix->orig;
    pf.n = (uint64_t)n;
    int *bad = nullptr;
    if (subset) {
        if (p->h_off_cap < nb + 1) {
            plan_drop_offsets(p);
            p->h_off = (int64_t *)malloc((size_t)(nb + 1) * 8);
            if (!p->h_off || hipMalloc((void **)&p->d_off, (size_t)(nb + 2) * 8) != hipSuccess) {
                p->d_off = nullptr;
                plan_drop_offsets(p);
                set_error("epoch_plan_build_positions: allocating %lld batch offsets failed", (long long)(nb + 1));
                return DAISY_ERR_HIP;
            }
            p->h_off_cap = nb + 1;
        }
        bad = (int *)(p->d_off + nb + 1);
        DAISY_HIP(hipMemsetAsync(bad, 0, 8, s));
        hipLaunchKernelGGL(k_positions_u32, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, perm, n, n_total, p->p_inv, bad);
        DAISY_LAUNCH_CHECK();
    } else if (order_mode == DAISY_ORDER_PERM) {
        hipLaunchKernelGGL(k_invert_perm, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, perm, n, p->p_inv);
        DAISY_LAUNCH_CHECK();
    }
    const BatchDiv bd = make_batch_div(batch_size);

    // (Round 5 ran the two partitions of a build - entry records, sample records - side by side on two streams, hoping
    // the VALU-bound counting kernels would hide under the scatters: every kernel took twice as long and the build as long
    // as before, 1.33 -> 1.36 ms per epoch at BASELINE configs[1] (profiles/r05_notes.txt).  The scatters are bound by
    // instruction issue like the counts - ranking by ballots, LDS sort - not by memory; deleted.)
    // per record kind (entries, then samples) and LSD digit: histogram of every tile, exclusive scan, stable scatter
    for (int what = 0; what < 2; ++what) {
        const bool entries = (what == 0);
        const int64_t m = entries ? ix->n_ent : n;
        int64_t tile_elems, ntiles;
        part_tiling(m, kPartThreads * (entries ? kPartKE : kPartK), tile_elems, ntiles);
        for (int pass = 0; pass < passes; ++pass) {
            const int shift = 8 * pass;
            const int bits_here = (bbits - shift < 8) ? (bbits - shift) : 8;
            const int64_t dig_here = (pass == passes - 1) ? ((nb - 1) >> shift) + 1 : 256;
            const int ndig = (int)(dig_here < 256 ? dig_here : 256);
            // LSD passes ping-pong between the record sets and end in set 0
            const int dset = ((passes - 1 - pass) & 1);
            const int sset = dset ^ 1;
            PartSrc src;
            memset(&src, 0, sizeof(src));
            src.triples = ix->triples; src.user_base = ix->user_base;
            src.ent_t = ix->ent_t; src.ent_key = ix->ent_key;
            src.srec = p->p_srec[sset]; src.erec = p->p_erec[sset];
            src.park = entries ? p->p_park : nullptr;
            const PartDst dst{p->p_srec[dset], p->p_erec[dset]};
            const dim3 g((unsigned)ntiles), b(kPartThreads);
#define DAISY_PART_COUNT(KIND)                                                                                      \
    hipLaunchKernelGGL((k_part_count<KIND>), g, b, 0, s, src, pf, bd, m, shift, bits_here, ndig, tile_elems, ntiles, \
                       p->p_counts)
            if (pass == 0) { if (entries) DAISY_PART_COUNT(1); else DAISY_PART_COUNT(0); }
            else { if (entries) DAISY_PART_COUNT(3); else DAISY_PART_COUNT(2); }
#undef DAISY_PART_COUNT
            DAISY_LAUNCH_CHECK();
            rc = exclusive_scan_u32(p->p_scan, p->p_scan_bytes, p->p_counts, p->p_offsets, (int64_t)ndig * ntiles, s);
            if (rc) return rc;
#define DAISY_PART_SCATTER(SAMPLES, STATIC, KK)                                                                      \
    hipLaunchKernelGGL((k_part_scatter<SAMPLES, STATIC, KK>), g, b, 0, s, src, pf, bd, m, shift, bits_here, ndig,      \
                       tile_elems, ntiles, p->p_offsets, 0u, dst)
            if (entries) { if (pass == 0) DAISY_PART_SCATTER(false, true, kPartKE); else DAISY_PART_SCATTER(false, false, kPartKE); }
            else { if (pass == 0) DAISY_PART_SCATTER(true, true, kPartK); else DAISY_PART_SCATTER(true, false, kPartK); }
#undef DAISY_PART_SCATTER
            DAISY_LAUNCH_CHECK();
        }
    }
    p->p_cur = 0;
    p->hot_item_share = ix->n_ent > 0 ? (double)ix->max_item_entries / (double)ix->n_ent : 0.0;
    p->n = n; p->batch_size = batch_size; p->num_batches = nb;
    p->pointwise = ix->pointwise;
    p->kind = 1;
    if (subset) {          // where every batch starts: one small copy and one host sync per epoch
        hipLaunchKernelGGL(k_batch_offsets, dim3(grid_for(nb + 1, kBlock)), dim3(kBlock), 0, s, p->p_srec[0], n, bd, nb,
                           p->d_off);
        DAISY_LAUNCH_CHECK();
        int bad_host[2] = {0, 0};
        if (hipMemcpyAsync(p->h_off, p->d_off, (size_t)(nb + 1) * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipMemcpyAsync(bad_host, bad, 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) {
            set_error("epoch_plan_build_positions: reading the batch offsets failed");
            p->built = false;
            return DAISY_ERR_HIP;
        }
        if (bad_host[0]) {
            set_error("epoch_plan_build_positions: a position lies outside [0, %lld)", (long long)n_total);
            p->built = false;
            return DAISY_ERR_ARG;
        }
    } else
        plan_drop_offsets(p);
    p->built = true;
    p->build_gen = next_plan_build_id();
    return DAISY_OK;
}

// Fills the index of `triples` (its scalar fields are set): `ix->keep` holds what the index keeps, `scratch` what only
// this call needs; the caller releases `scratch`, and `ix->keep` too when the call fails.
static int index_build(daisy_train_index *ix, DeviceArena &scratch, const int32_t *triples, bool sorted, hipStream_t s) {
    const int64_t n = ix->n, user_num = ix->U, item_num = ix->I;
    const int32_t user_base = ix->user_base, pointwise = ix->pointwise;
    // scratch: unsorted entry pairs [2n] x2, (unsorted user pairs [n] x2 + sorted keys [n]), bad flag, sort temp, item bounds
    const size_t t_sort = sort_pairs_i32_temp_bytes(2 * n);
    uint32_t *k, *v, *uk, *uv, *uk2, *hist;
    int *bad;
    void *tmp;
    scratch.add(&k, (size_t)n * 8); scratch.add(&v, (size_t)n * 8);
    scratch.add(&uk, (size_t)n * 4); scratch.add(&uv, (size_t)n * 4); scratch.add(&uk2, (size_t)n * 4);
    scratch.add(&bad, 256); scratch.add(&tmp, t_sort); scratch.add(&hist, (size_t)item_num * 8);
    DeviceArena &keep = ix->keep;
    keep.add(&ix->ent_t, (size_t)n * 8); keep.add(&ix->ent_key, (size_t)n * 8);
    if (!sorted) { keep.add(&ix->sorted_copy, (size_t)n * 12); keep.add(&ix->orig, (size_t)n * 4); }
    int rc;
    if ((rc = scratch.alloc("train_index_create")) || (rc = keep.alloc("train_index_create"))) return rc;
    if (hipMemsetAsync(bad, 0, 8, s) != hipSuccess) return DAISY_ERR_HIP;
    const int32_t *src = triples;
    if (!sorted) {   // CSR order first: stable sort of the row indices by user, then one gather
        hipLaunchKernelGGL(k_index_entries, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, triples, n, user_base,
                           user_num, item_num, (uint32_t *)nullptr, (uint32_t *)nullptr, uk, uv, bad, pointwise);
        rc = sort_pairs_i32(tmp, t_sort, (const int32_t *)uk, (int32_t *)uk2, (const int32_t *)uv,
                            (int32_t *)ix->orig, n, bits_for(user_num), s);
        if (rc) return rc;
        hipLaunchKernelGGL(k_gather_triples, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, triples, ix->orig, n,
                           ix->sorted_copy);
        src = ix->sorted_copy;
    }
    ix->triples = src;
    hipLaunchKernelGGL(k_index_entries, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, src, n, user_base, user_num,
                       item_num, k, v, (uint32_t *)nullptr, (uint32_t *)nullptr, bad, pointwise);
    rc = sort_pairs_i32(tmp, t_sort, (const int32_t *)k, (int32_t *)ix->ent_key, (const int32_t *)v,
                        (int32_t *)ix->ent_t, ix->n_ent, bits_for(item_num) + 1, s);
    if (rc) return rc;
    // (bad[1]: entries of the most frequent item; out-of-range items were replaced by 0 and are reported below)
    if (hipMemsetAsync(hist, 0, (size_t)item_num * 8, s) != hipSuccess) return DAISY_ERR_HIP;
    hipLaunchKernelGGL(k_item_bounds, dim3(grid_for(ix->n_ent, kBlock * 4)), dim3(kBlock), 0, s, ix->ent_key, ix->n_ent, hist,
                       hist + item_num);
    hipLaunchKernelGGL(k_item_max_len, dim3(grid_for(item_num, kBlock * 4, 256)), dim3(kBlock), 0, s, hist, hist + item_num,
                       item_num, (uint32_t *)(bad + 1));
    int bad_host[2] = {0, 0};
    if (hipMemcpyAsync(bad_host, bad, 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        set_error("train_index_create: reading the validation flag failed");
        return DAISY_ERR_HIP;
    }
    ix->max_item_entries = (int64_t)(uint32_t)bad_host[1];
    if (bad_host[0]) {
        set_error("index out of range in the training triples: need %d <= user < %lld and 0 <= item < %lld "
                  "(the reference raises IndexError in nn.Embedding, MFRecommender.py:64-65)",
                  user_base, (long long)(user_base + user_num), (long long)item_num);
        return DAISY_ERR_ARG;
    }
    return DAISY_OK;
}

// what the last sorted build (`who` names the entry point that ran it) found wrong with its ids: one host sync
int plan_report_bad(const daisy_epoch_plan *p, const char *who, hipStream_t s) {
    int bad = 0;
    DAISY_HIP(hipMemcpyAsync(&bad, p->bad, sizeof(int), hipMemcpyDeviceToHost, s));
    DAISY_HIP(hipStreamSynchronize(s));
    if (bad & 2) { set_error("%s: index out of range in the epoch permutation", who); return DAISY_ERR_ARG; }
    if (bad & 1) {
        set_error("%s: index out of range in the batch: need 0 <= user - user_base < %lld and 0 <= item < %lld "
                  "(the reference raises IndexError in nn.Embedding, MFRecommender.py:64-65)", who, (long long)p->U,
                  (long long)p->I);
        return DAISY_ERR_ARG;
    }
    return DAISY_OK;
}

}  // namespace daisy

using namespace daisy;

// =============================================================================
// C ABI
// =============================================================================
extern "C" {

int daisy_epoch_plan_create(daisy_epoch_plan **out, int64_t max_triples, int64_t user_num,
                            int64_t item_num) {
    DAISY_CHECK_ARG(out != nullptr, "epoch_plan_create: out is NULL");
    DAISY_CHECK_ARG(max_triples > 0 && max_triples < ((int64_t)1 << 30),
                    "epoch_plan_create: max_triples=%lld out of range", (long long)max_triples);
    DAISY_CHECK_ARG(user_num > 0 && user_num <= INT32_MAX && item_num > 0 && item_num <= INT32_MAX,
                    "epoch_plan_create: user_num/item_num out of int32 range");
    return plan_alloc(out, max_triples, user_num, item_num);
}

int daisy_epoch_plan_destroy(daisy_epoch_plan *plan) { return plan ? plan_free(plan) : DAISY_OK; }

size_t daisy_epoch_plan_bytes(const daisy_epoch_plan *plan) { return plan ? plan_bytes(plan) : 0; }

int64_t daisy_epoch_plan_num_batches(const daisy_epoch_plan *plan) { return (plan && plan->built) ? plan->num_batches : 0; }

int daisy_epoch_plan_build(daisy_epoch_plan *plan, const int32_t *triples, int64_t n_triples,
                           const int64_t *perm, int32_t order_mode, uint64_t seed, uint64_t epoch,
                           int64_t batch_size, int32_t user_base, int32_t flags,
                           daisy_stream_t stream) {
    DAISY_CHECK_ARG(plan && triples, "epoch_plan_build: NULL argument");
    DAISY_CHECK_ARG(n_triples > 0 && n_triples <= plan->max_triples,
                    "epoch_plan_build: n_triples=%lld not in 1..%lld", (long long)n_triples,
                    (long long)plan->max_triples);
    DAISY_CHECK_ARG(batch_size > 0, "epoch_plan_build: batch_size must be positive");
    DAISY_CHECK_ARG(order_mode >= DAISY_ORDER_IDENTITY && order_mode <= DAISY_ORDER_FEISTEL,
                    "epoch_plan_build: bad order_mode %d", order_mode);
    DAISY_CHECK_ARG(order_mode != DAISY_ORDER_PERM || perm != nullptr,
                    "epoch_plan_build: DAISY_ORDER_PERM needs perm");
    return plan_build(plan, triples, n_triples, 0, perm, order_mode, seed, epoch, batch_size, user_base,
                      flags, as_stream(stream));
}

int daisy_epoch_plan_validate(const daisy_epoch_plan *plan, daisy_stream_t stream) {
    DAISY_CHECK_ARG(plan != nullptr, "epoch_plan_validate: NULL plan");
    if (!plan->built) { set_error("epoch_plan_validate: plan has not been built"); return DAISY_ERR_STATE; }
    if (plan->kind == 1) return DAISY_OK;            // a train index is validated when it is created
    return plan_report_bad(plan, "epoch_plan_build", as_stream(stream));
}

int daisy_epoch_plan_read_batch(const daisy_epoch_plan *plan, int64_t k, int32_t *u, int32_t *i,
                                int32_t *j, int32_t *ent_item, uint32_t *ent_s, int32_t *ent_u,
                                int64_t *B_out_host, daisy_stream_t stream) {
    DAISY_CHECK_ARG(plan && u && i && j, "epoch_plan_read_batch: NULL argument");
    if (!plan->built) { set_error("epoch_plan_read_batch: plan has not been built"); return DAISY_ERR_STATE; }
    DAISY_CHECK_ARG(k >= 0 && k < plan->num_batches, "epoch_plan_read_batch: batch %lld not in 0..%lld",
                    (long long)k, (long long)plan->num_batches);
    if (plan->kind == 1) return plan_read_batch_partitioned(plan, k, u, i, j, ent_item, ent_s, ent_u, B_out_host, as_stream(stream));
    const BatchView v = plan_view(plan, k);
    hipLaunchKernelGGL(k_unpack_batch, dim3(grid_for(2 * v.B, kBlock)), dim3(kBlock), 0, as_stream(stream), v, u, i,
                       j, ent_item, ent_s, ent_u);
    DAISY_LAUNCH_CHECK();
    if (B_out_host) *B_out_host = v.B;
    return DAISY_OK;
}

int daisy_feistel_positions(int64_t n, uint64_t seed, uint64_t epoch, int64_t *out,
                            daisy_stream_t stream) {
    DAISY_CHECK_ARG(out && n > 0 && n <= ((int64_t)1 << 30), "feistel_positions: n must be in 1..2^30");
    FeistelKey fk = make_feistel_key((uint64_t)n, seed, epoch);
    hipLaunchKernelGGL(k_feistel_perm, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, as_stream(stream), n, fk, out);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_feistel_positions_at(const int64_t *ids, int64_t n_ids, int64_t n, uint64_t seed, uint64_t epoch,
                               int64_t *out, daisy_stream_t stream) {
    DAISY_CHECK_ARG(ids && out && n_ids > 0 && n > 0 && n <= ((int64_t)1 << 30), "feistel_positions_at: bad argument");
    FeistelKey fk = make_feistel_key((uint64_t)n, seed, epoch);
    hipLaunchKernelGGL(k_feistel_at, dim3(grid_for(n_ids, kBlock)), dim3(kBlock), 0, as_stream(stream), ids, n_ids, n, fk, out);
    DAISY_LAUNCH_CHECK();
    return DAISY_OK;
}

int daisy_train_index_create(daisy_train_index **out, const int32_t *triples, int64_t n_triples, int64_t user_num,
                             int64_t item_num, int32_t user_base, int32_t flags, daisy_stream_t stream) {
    DAISY_CHECK_ARG(out && triples, "train_index_create: NULL argument");
    DAISY_CHECK_ARG(n_triples > 0 && n_triples < ((int64_t)1 << 30), "train_index_create: n_triples=%lld out of range",
                    (long long)n_triples);
    DAISY_CHECK_ARG(user_num > 0 && user_num <= INT32_MAX && item_num > 0 && item_num < ((int64_t)1 << 30),
                    "train_index_create: user_num/item_num out of range");
    daisy_train_index *ix = new daisy_train_index();      // (all zero)
    ix->n = n_triples; ix->U = user_num; ix->I = item_num; ix->user_base = user_base;
    ix->pointwise = (flags & DAISY_PLAN_POINTWISE) ? 1 : 0;
    ix->n_ent = ix->pointwise ? n_triples : 2 * n_triples;
    DeviceArena scratch;
    const int rc = index_build(ix, scratch, triples, (flags & DAISY_PLAN_TRIPLES_USER_SORTED) != 0, as_stream(stream));
    (void)scratch.release();
    if (rc) {
        (void)ix->keep.release();
        delete ix;
        return rc;
    }
    *out = ix;
    return DAISY_OK;
}

int daisy_train_index_destroy(daisy_train_index *index) {
    if (!index) return DAISY_OK;
    const hipError_t e = index->keep.release() ? hipSuccess : hipGetLastError();
    delete index;
    if (e != hipSuccess) {
        set_error("train_index_destroy: hipFree failed: %s", hipGetErrorString(e));
        return DAISY_ERR_HIP;
    }
    return DAISY_OK;
}

size_t daisy_train_index_bytes(const daisy_train_index *index) { return index ? index->keep.bytes() : 0; }

int daisy_epoch_plan_build_indexed(daisy_epoch_plan *plan, const daisy_train_index *index, const int64_t *perm,
                                   int32_t order_mode, uint64_t seed, uint64_t epoch, int64_t batch_size,
                                   daisy_stream_t stream) {
    DAISY_CHECK_ARG(plan && index, "epoch_plan_build_indexed: NULL argument");
    DAISY_CHECK_ARG(index->n <= plan->max_triples && index->U == plan->U && index->I == plan->I,
                    "epoch_plan_build_indexed: the index (n %lld, U %lld, I %lld) does not fit the plan",
                    (long long)index->n, (long long)index->U, (long long)index->I);
    DAISY_CHECK_ARG(batch_size > 0 && batch_size < ((int64_t)1 << 31), "epoch_plan_build_indexed: bad batch_size");
    DAISY_CHECK_ARG(order_mode >= DAISY_ORDER_IDENTITY && order_mode <= DAISY_ORDER_FEISTEL,
                    "epoch_plan_build_indexed: bad order_mode %d", order_mode);
    DAISY_CHECK_ARG(order_mode != DAISY_ORDER_PERM || perm != nullptr,
                    "epoch_plan_build_indexed: DAISY_ORDER_PERM needs perm");
    return plan_build_partitioned(plan, index, perm, order_mode, seed, epoch, batch_size, 0, as_stream(stream));
}

int daisy_epoch_plan_build_positions(daisy_epoch_plan *plan, const daisy_train_index *index, const int64_t *positions,
                                     int64_t n_total, int64_t batch_size, daisy_stream_t stream) {
    DAISY_CHECK_ARG(plan && index && positions, "epoch_plan_build_positions: NULL argument");
    DAISY_CHECK_ARG(index->n <= plan->max_triples && index->U == plan->U && index->I == plan->I,
                    "epoch_plan_build_positions: the index (n %lld, U %lld, I %lld) does not fit the plan",
                    (long long)index->n, (long long)index->U, (long long)index->I);
    DAISY_CHECK_ARG(batch_size > 0 && batch_size < ((int64_t)1 << 31), "epoch_plan_build_positions: bad batch_size");
    DAISY_CHECK_ARG(n_total >= index->n && n_total < ((int64_t)1 << 32),
                    "epoch_plan_build_positions: n_total=%lld must be in [n, 2^32)", (long long)n_total);
    return plan_build_partitioned(plan, index, positions, DAISY_ORDER_PERM, 0, 0, batch_size, n_total, as_stream(stream));
}

int64_t daisy_epoch_plan_batch_rows(const daisy_epoch_plan *plan, int64_t k) {
    if (!plan || !plan->built || k < 0 || k >= plan->num_batches) return -1;
    if (plan->h_off) return plan->h_off[k + 1] - plan->h_off[k];
    const int64_t lo = k * plan->batch_size;
    return (plan->n - lo < plan->batch_size) ? (plan->n - lo) : plan->batch_size;
}

}  // extern "C"
