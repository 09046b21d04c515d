// What the bank's translation units share (search.hip, pool.hip, gram.hip): the bits of the bank's err word, the packed fp16
// types, the exact widening of e4m3fn codes, and the CSR groups of the pool and the Gram matrix cut into chunks.
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

// entries [a, b) of group g, clamped so that nothing is read out of bounds whatever `starts` holds (the scan below reports it)
__device__ inline void bank_group_range(const int64_t* __restrict__ starts, int64_t g, int64_t L, int64_t& a, int64_t& b) {
    a = starts[g];
    b = starts[g + 1];
    a = a < 0 ? 0 : (a > L ? L : a);
    b = b < a ? a : (b > L ? L : b);
}

constexpr int BANK_SCAN_T = 1024;  // threads of the one scan workgroup

// A group is cut into chunks of C consecutive entries: chunk_base[g] = the number of chunks of the groups before g;
// chunk_base[G] = all chunks.  One workgroup.
template <int C>
__global__ __launch_bounds__(BANK_SCAN_T) void bank_chunk_scan_kernel(const int64_t* __restrict__ starts, int64_t G, int64_t L,
                                                                      int64_t* __restrict__ chunk_base, int32_t* __restrict__ err) {
    __shared__ int64_t sh[BANK_SCAN_T];
    const int tid = threadIdx.x;
    int64_t carry = 0;
    for (int64_t g0 = 0; g0 < G; g0 += BANK_SCAN_T) {
        const int64_t g = g0 + tid;
        int64_t c = 0;
        if (g < G) {
            const int64_t sa = starts[g], sb = starts[g + 1];
            if (sa < 0 || sb < sa || sb > L || (g == 0 && sa != 0) || (g == G - 1 && sb != L)) atomicOr(err, BANK_E_POOL_STARTS);
            int64_t a, b;
            bank_group_range(starts, g, L, a, b);
            c = (b - a + C - 1) / C;
        }
        sh[tid] = c;
        __syncthreads();
        for (int o = 1; o < BANK_SCAN_T; o <<= 1) {
            const int64_t v = sh[tid] + (tid >= o ? sh[tid - o] : 0);
            __syncthreads();
            sh[tid] = v;
            __syncthreads();
        }
        if (g < G) chunk_base[g] = carry + sh[tid] - c;
        carry += sh[BANK_SCAN_T - 1];
        __syncthreads();
    }
    if (tid == 0) chunk_base[G] = carry;
}

}  // namespace osn
