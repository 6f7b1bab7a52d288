// MFMA fragment types, the bf16 conversions and gfx950's transposing LDS fragment read: shared by every file that feeds
// the matrix cores (gemm.hip, the NeuMF kernels, ngcf.hip).
#pragma once
#include "common.h"

namespace daisy {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t bf16_rne(float f) {
    uint32_t u = __float_as_uint(f);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ float bf16_to_f32(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
// two floats -> two bf16 (round to nearest even) in one dword, lo in bits 0..15: gfx950's v_cvt_pk_bf16_f32 - one
// instruction where the integer form above takes five per value (the epilogue of a 128x128 tile converts 64 values
// per lane: that was more VALU work than the tile's MFMAs at K = 128)
__device__ __forceinline__ uint32_t bf16_pack2(float lo, float hi) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

__device__ __forceinline__ bool bf16_positive(uint16_t h) { return (h & 0x8000u) == 0 && (h & 0x7FFFu) != 0; }

// An operand that is contiguous along its ROWS instead of k is copied to LDS as it lies in memory - [k][row] tiles - and
// the MFMA fragment (8 consecutive k of one row per lane) comes out of gfx950's transposing LDS read: ds_read_b64_tr_b16
// hands lane i of a 16-lane group column i of the [4 k][16 rows] block whose 16 four-element pieces the lanes address
// (measured: result[i][j] = piece[4j + i/4][i%4]), two of them per fragment (p: this lane's piece for k rows 0..3 of its
// half, the second piece 4 k rows = 4 * pitch halfwords further).
typedef short short4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ bf16x8 lds_frag_tr(const uint16_t *p, int pitch) {
    typedef __attribute__((address_space(3))) short4v *lds_v4;
    const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)p);
    const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(p + 4 * pitch));
    typedef short short8v __attribute__((ext_vector_type(8)));
    const short8v v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

// the second piece at an address of its own (swizzled layouts: the k rows 4 apart do not differ by a fixed stride)
__device__ __forceinline__ bf16x8 lds_frag_tr2(const uint16_t *p_lo, const uint16_t *p_hi) {
    typedef __attribute__((address_space(3))) short4v *lds_v4;
    const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)p_lo);
    const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)p_hi);
    typedef short short8v __attribute__((ext_vector_type(8)));
    const short8v v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

}  // namespace daisy
