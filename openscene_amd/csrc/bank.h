// What the bank's translation units share (search.hip, pool.hip, gram.hip, match.hip): the bits of the bank's err word, the
// packed fp16 types, the exact widening of e4m3fn codes, the fp16 operand of a row (its fp32 factor and the rounding: the Gram
// matrix and the matcher take bit for bit the same), and the CSR groups of the pool and the Gram matrix cut into chunks.
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

// The factor of a stored row: 2^e / (||c|| 2^e + 1e-5) (fp16 rows: 2^e = sc = 1), or 2^e alone when the rows are taken as they
// are stored.  One wave per row, every lane calls it and every lane receives the factor: lane l squares the 16-byte groups
// l, l + 64, .. in order and the 64 partial sums meet in a butterfly -- the pool's reduction.
template <bool FP8>
__device__ __forceinline__ float bank_row_factor(const char* __restrict__ row, int d, float sc, int normalize, int lane) {
    if (!normalize) return sc;
    const int ng = d / (FP8 ? 16 : 8);
    float ss = 0.f;
    for (int grp = lane; grp < ng; grp += 64) {
        const uint4 raw = *reinterpret_cast<const uint4*>(row + int64_t(grp) * 16);
        if (FP8) {
            half2 h[8];
            q8_widen(raw, h);
#pragma unroll
            for (int k = 0; k < 8; ++k) { ss = fmaf((float)h[k][0], (float)h[k][0], ss); ss = fmaf((float)h[k][1], (float)h[k][1], ss); }
        } else {
            const half8 h = __builtin_bit_cast(half8, raw);
#pragma unroll
            for (int k = 0; k < 8; ++k) ss = fmaf((float)h[k], (float)h[k], ss);
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
    return sc / (sqrtf(ss) * sc + 1e-5f);
}

// 2^e of an fp8 row's exponent byte
__device__ __forceinline__ float bank_exp2(int8_t e) { return __uint_as_float(uint32_t(127 + int(e)) << 23); }

// the operand of eight stored values (widened exactly to fp16) under the row's factor: fp16_rne(v * s), the product in fp32
__device__ __forceinline__ half8 bank_round8(const half8& v, float s) {
    half8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = (_Float16)((float)v[k] * s);
    return o;
}

// scale[i] = bank_row_factor of entry i's row (0 for a row outside the bank, which the caller skips and reports); one wave
// per entry
template <bool FP8>
__global__ __launch_bounds__(256) void bank_scale_kernel(const void* __restrict__ B, const int8_t* __restrict__ E, int64_t n, int d,
                                                         const int64_t* __restrict__ rows, int64_t L, int normalize,
                                                         float* __restrict__ scale) {
    const int lane = threadIdx.x & 63;
    const int64_t i = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (i >= L) return;
    const int64_t r = rows ? rows[i] : i;
    if (r < 0 || r >= n) {
        if (lane == 0) scale[i] = 0.f;
        return;
    }
    const float f = bank_row_factor<FP8>(static_cast<const char*>(B) + r * int64_t(d) * (FP8 ? 1 : 2), d, FP8 ? bank_exp2(E[r]) : 1.f,
                                         normalize, lane);
    if (lane == 0) scale[i] = f;
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
