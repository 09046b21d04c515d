// What the bank's translation units share (search.hip, pool.hip): the bits of the bank's err word, the packed fp16 types and
// the exact widening of e4m3fn codes.
#pragma once
#include "common.h"

namespace osn {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half2 __attribute__((ext_vector_type(2)));

// bits of the bank's err word (osn_bank_check spells them out)
constexpr int BANK_E_GATHER = 1, BANK_E_OFFSETS = 2, BANK_E_LONG = 4;
constexpr int BANK_E_POOL_ROW = 8, BANK_E_POOL_WEIGHT = 16, BANK_E_POOL_STARTS = 32;

// 16 e4m3fn codes (one 16-byte load) -> 16 fp16 values in code order; e4m3 -> fp16 is exact (v_cvt_scalef32_pk_f16_fp8, scale 1)
__device__ __forceinline__ void q8_widen(const uint4& v, half2 (&h)[8]) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        h[2 * j] = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[j], 1.0f, false);
        h[2 * j + 1] = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[j], 1.0f, true);
    }
}

}  // namespace osn
