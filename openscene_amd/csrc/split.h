// The split-bf16 ("bf16x6") arithmetic of the convolution kernels, stated once: the three bf16 pieces of an fp32
// operand, the MFMA operand types, and the six cross products a kernel keeps, in their order.
#pragma once
#include "common.h"
#include <type_traits>

namespace osn {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef bf16x4 split_bf16x4;      // earlier name of bf16x4 (tools/probes/spconv_pl.hip)

// v = h1 + h2 + h3 with three bf16 pieces, each the round-to-nearest bf16 of what the pieces before it left over
// (tests/conv_bounds.py split3).  tl_split4 below computes the same three pieces, two elements per conversion.
__device__ __forceinline__ void split1(float v, __bf16& h1, __bf16& h2, __bf16& h3) {
    h1 = (__bf16)v;
    const float r1 = v - (float)h1;
    h2 = (__bf16)r1;
    h3 = (__bf16)(r1 - (float)h2);
}

// fp32 x 4 -> the three bf16 pieces of every element (x = h1 + h2 + h3 exactly; round to nearest), two elements per instruction
__device__ __forceinline__ void tl_split4(const float4 x, bf16x4& p1, bf16x4& p2, bf16x4& p3) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    typedef uint32_t u2 __attribute__((ext_vector_type(2)));
    const f2 v[2] = {f2{x.x, x.y}, f2{x.z, x.w}};
    u2 q1, q2, q3;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const b2 h1 = __builtin_convertvector(v[j], b2);
        const uint32_t u1 = __builtin_bit_cast(uint32_t, h1);
        const f2 r1 = v[j] - f2{__builtin_bit_cast(float, u1 << 16), __builtin_bit_cast(float, u1 & 0xFFFF0000u)};
        const b2 h2 = __builtin_convertvector(r1, b2);
        const uint32_t u2_ = __builtin_bit_cast(uint32_t, h2);
        const f2 r2 = r1 - f2{__builtin_bit_cast(float, u2_ << 16), __builtin_bit_cast(float, u2_ & 0xFFFF0000u)};
        const b2 h3 = __builtin_convertvector(r2, b2);
        q1[j] = u1; q2[j] = u2_; q3[j] = __builtin_bit_cast(uint32_t, h3);
    }
    p1 = __builtin_bit_cast(bf16x4, q1);
    p2 = __builtin_bit_cast(bf16x4, q2);
    p3 = __builtin_bit_cast(bf16x4, q3);
}

// The eight-wide MFMA operand fragment of eight fp32 values: piece[p] = piece p of (lo, hi)
__device__ __forceinline__ void split8(const float4 lo, const float4 hi, bf16x8 (&piece)[3]) {
    bf16x4 l[3], h[3];
    tl_split4(lo, l[0], l[1], l[2]);
    tl_split4(hi, h[0], h[1], h[2]);
#pragma unroll
    for (int p = 0; p < 3; ++p) piece[p] = __builtin_shufflevector(l[p], h[p], 0, 1, 2, 3, 4, 5, 6, 7);
}

// The six products kept of the nine (tests/conv_bounds.py KEPT; pieces counted from 0 here, and those with
// a + b > 2 are dropped: <= 2^-24 relative): f(a piece, b piece) is called in the order in which every kernel adds
// them to any ONE accumulator -- a3b1, a2b2, a1b3, a2b1, a1b2, a1b1, smallest terms first, so that the small ones meet
// a small sum and are not rounded away against a1b1.  A kernel that loops over its accumulators INSIDE f keeps
// consecutive MFMAs on different accumulators.  The indices are compile-time constants that convert to int, so
// operands indexed by them stay in registers.
template <class F>
__device__ __forceinline__ void split_products(F&& f) {
    using std::integral_constant;
    f(integral_constant<int, 2>{}, integral_constant<int, 0>{});
    f(integral_constant<int, 1>{}, integral_constant<int, 1>{});
    f(integral_constant<int, 0>{}, integral_constant<int, 2>{});
    f(integral_constant<int, 1>{}, integral_constant<int, 0>{});
    f(integral_constant<int, 0>{}, integral_constant<int, 1>{});
    f(integral_constant<int, 0>{}, integral_constant<int, 0>{});
}

}  // namespace osn
