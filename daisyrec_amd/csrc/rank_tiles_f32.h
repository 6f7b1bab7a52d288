// What the two kernels on the fp32 MFMA tile stream share by name (DESIGN.md sections 24 and 27): k_full_rank_tiles
// (rank_full.hip) appends a tile's sort words to per-user candidate lists, k_frp_count (rank_positions.hip) counts
// the tile's sort words above each target's.  Both score 64 columns (users, or slots of a user's targets) against a
// slice of whole 128-item tiles, and both must see the same score bits, masks and tiles: the tile geometry, the slice
// arithmetic and the small device helpers live here, once.
//
// The chunk stream itself - register ring, LDS stages, MFMA chain, exclusion walk - is NOT here: it stands in each
// kernel, as lambdas over the kernel's locals.  Two shared forms were built and measured against the two copies.  A
// function template taking the epilogue as a callable kept the registers, but the workgroup-size query inside the
// list epilogue's __syncthreads_or was no longer folded away: inlined through the function it came out as global
// loads at every tile, each a vmcnt(0) that drains the chunks in flight.  A struct driven from the kernel kept the
// fold, but the compiler filled all 256 VGPRs of the list kernel and parked 8 more values in AGPRs, the count kernel
// came within 2 registers of losing its second wave, and both ran 0.7 to 3.7 % slower.  Whoever changes the loop in one
// kernel changes it in the other: rank_positions.hip says so at its copy.
#pragma once

#include "common.h"

namespace daisy {

constexpr int kRtBM = 128;                      // items per tile (MFMA M side)
constexpr int kRtBN = 64;                       // columns per tile (MFMA N side): users, or slots
constexpr int kRtBK = 16;                       // k depth of an LDS tile
constexpr int kRtLA = kRtBM + 4, kRtLB = kRtBN + 4;
constexpr int kRtAhead = 4;                     // chunks in flight from memory ahead of the one in LDS
constexpr int kRtStageBytes = 2 * kRtBK * (kRtLA + kRtLB) * 4;     // As [2][kRtBK * kRtLA] and Bs [2][kRtBK * kRtLB]
constexpr int kRtMaskBytes = kRtBN * 4 * 4;     // one mask buffer: [64 columns][4 words], bit = item of the tile
static_assert(kRtBN * 4 == kBlock, "a thread of the quad walk writes one mask word");

__device__ __forceinline__ uint64_t rt_shfl_xor(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, kWave);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, kWave);
    return ((uint64_t)hi << 32) | lo;
}

// the item of a 32-item block that accumulator element i of this lane holds (the lane's column is lane % 32): the
// C/D map of the 32x32 MFMA, the one gemm_epilogue decodes
__device__ __forceinline__ int rt_acc_item(int i, int lane) { return (i / 4) * 8 + (lane / 32) * 4 + (i % 4); }

// first position in [a, b) of an ascending exclusion row whose entry is not below v.  Contents are only compared, so
// an unsorted row costs exclusions, no more.
__device__ __forceinline__ int64_t rt_lower_bound(const int32_t *__restrict__ eitems, int64_t a, int64_t b, int64_t v) {
    while (a < b) {
        const int64_t m = a + (b - a) / 2;
        if ((int64_t)eitems[m] < v) a = m + 1;
        else b = m;
    }
    return a;
}

// item slices of a call: whole 128-item tiles, every slice non-empty.  requested 0: as many as bring the grid of
// `cols` columns to about target_groups workgroups.
static inline void rt_slices(int64_t cols, int64_t item_num, int32_t requested, int target_groups, int64_t *tiles_per_slice,
                             int64_t *n_tiles, int *S) {
    const int64_t T = (item_num + kRtBM - 1) / kRtBM, UT = (cols + kRtBN - 1) / kRtBN;
    int64_t want = requested > 0 ? requested : (target_groups / UT > 1 ? target_groups / UT : 1);
    if (want > T) want = T;
    const int64_t per = (T + want - 1) / want;
    *tiles_per_slice = per;
    *n_tiles = T;
    *S = (int)((T + per - 1) / per);
}

// VEC of the tile kernels: rows of both tables are whole, aligned float4s
static inline bool rt_vec(int d, const float *P, const float *Q) {
    return (d % 4 == 0) && (reinterpret_cast<uintptr_t>(P) % 16 == 0) && (reinterpret_cast<uintptr_t>(Q) % 16 == 0);
}

}  // namespace daisy
