// The order-preserving 32-bit key of an fp32 score, shared by the full rankings on fp32 scores (rank_full.hip, DESIGN.md
// section 24; rank_rows.hip, section 26) and their positions kernels (sections 27 and 28).  Their 64-bit sort word,
// fr_word, is (fr_key(v) << 32) | (0xFFFFFFFF - item): a plain unsigned maximum is then the order (score descending, a
// NaN first, -0.0 equal to +0.0, equal scores by ascending item id), and no candidate maps to word 0.
#pragma once

#include "common.h"

namespace daisy {

// order-preserving key of a score: larger score <-> larger key; NaN is the largest (torch.argsort(descending=True)
// puts it first); v + 0.0f makes -0.0 and +0.0 one key
__device__ __forceinline__ uint32_t fr_key(float v) {
    v = v + 0.0f;
    if (v != v) return 0xFFFFFFFFu;
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float fr_unkey(uint32_t key) {
    if (key == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// the sort word of (score, item) and its two halves back
__device__ __forceinline__ uint64_t fr_word(float v, int64_t item) {
    return ((uint64_t)fr_key(v) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)item);
}
__device__ __forceinline__ int64_t fr_word_item(uint64_t w) { return (int64_t)(0xFFFFFFFFu - (uint32_t)w); }
__device__ __forceinline__ float fr_word_score(uint64_t w) { return fr_unkey((uint32_t)(w >> 32)); }

}  // namespace daisy
