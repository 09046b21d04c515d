// The split-bf16 arithmetic of the convolution kernels, stated once: the bf16 pieces of an fp32 operand, the MFMA operand
// types, and the cross products a kernel keeps, in their order -- for three pieces ("bf16x6": six products, fp32-class, the default)
// and for the reduced inference modes of two ("bf16x3") and one ("bf16x1").
#pragma once
#include "common.h"
#include <type_traits>

namespace osn {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef bf16x4 split_bf16x4;      // earlier name of bf16x4 (tools/probes/spconv_pl.hip)

// ---- the piece count NP of a kernel instance (3 = "bf16x6", the default and everything training runs; 2 = "bf16x3" and
// 1 = "bf16x1", the reduced inference modes).  NP selects BOTH the leading pieces an operand is split into and the products kept:
//     h_i(a) h_j(b) is kept  iff  i + j <= NP + 1   (pieces counted from 1)
//     NP = 3: 31 22 13 21 12 11      NP = 2: 21 12 11      NP = 1: 11      in this order, smallest first, into fp32.
// The first NP pieces of an operand are the same values whatever NP is (piece p depends only on the pieces before it), so a reduced
// instance reads planes 0 .. NP - 1 of the same weight image.  Dropped products, per term of |a||b| (|h2| <= 2^-8, |h3| <= 2^-17 of
// the operand): NP = 2 loses 22 + 13 + 31 <= 2^-16 + 2 * 2^-17 = 2^-15; NP = 1 also loses 12 + 21 <= 2 * 2^-8 = 2^-7 (plus terms of
// 2^-16 and below that the fp32 accumulation budget covers) -- tests/conv_pieces.py holds the kernels to both.

// v = h1 + h2 + h3 with three bf16 pieces, each the round-to-nearest bf16 of what the pieces before it left over
// (tests/conv_bounds.py split3): the first NP of them.  NP = 1 is one round-to-nearest conversion.
template <int NP>
__device__ __forceinline__ void split1(float v, __bf16 (&h)[NP]) {
    static_assert(NP >= 1 && NP <= 3, "one to three pieces");
    const __bf16 h1 = (__bf16)v;
    h[0] = h1;
    if constexpr (NP > 1) {
        const float r1 = v - (float)h1;
        const __bf16 h2 = (__bf16)r1;
        h[1] = h2;
        if constexpr (NP > 2) h[2] = (__bf16)(r1 - (float)h2);
    }
}
__device__ __forceinline__ void split1(float v, __bf16& h1, __bf16& h2, __bf16& h3) {
    __bf16 h[3];
    split1<3>(v, h);
    h1 = h[0]; h2 = h[1]; h3 = h[2];
}

// fp32 x 4 -> the first NP bf16 pieces of every element (NP = 3: x = p[0] + p[1] + p[2] exactly; round to nearest), two elements
// per instruction
template <int NP>
__device__ __forceinline__ void tl_split4(const float4 x, bf16x4 (&p)[NP]) {
    static_assert(NP >= 1 && NP <= 3, "one to three pieces");
    typedef float f2 __attribute__((ext_vector_type(2)));
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    typedef uint32_t u2 __attribute__((ext_vector_type(2)));
    const f2 v[2] = {f2{x.x, x.y}, f2{x.z, x.w}};
    u2 q[NP];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const b2 h1 = __builtin_convertvector(v[j], b2);
        const uint32_t u1 = __builtin_bit_cast(uint32_t, h1);
        q[0][j] = u1;
        if constexpr (NP > 1) {
            const f2 r1 = v[j] - f2{__builtin_bit_cast(float, u1 << 16), __builtin_bit_cast(float, u1 & 0xFFFF0000u)};
            const b2 h2 = __builtin_convertvector(r1, b2);
            const uint32_t u2_ = __builtin_bit_cast(uint32_t, h2);
            q[1][j] = u2_;
            if constexpr (NP > 2) {
                const f2 r2 = r1 - f2{__builtin_bit_cast(float, u2_ << 16), __builtin_bit_cast(float, u2_ & 0xFFFF0000u)};
                const b2 h3 = __builtin_convertvector(r2, b2);
                q[2][j] = __builtin_bit_cast(uint32_t, h3);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) p[i] = __builtin_bit_cast(bf16x4, q[i]);
}
__device__ __forceinline__ void tl_split4(const float4 x, bf16x4& p1, bf16x4& p2, bf16x4& p3) {
    bf16x4 p[3];
    tl_split4<3>(x, p);
    p1 = p[0]; p2 = p[1]; p3 = p[2];
}

// The eight-wide MFMA operand fragment of eight fp32 values: piece[p] = piece p of (lo, hi), p < NP
template <int NP>
__device__ __forceinline__ void split8(const float4 lo, const float4 hi, bf16x8 (&piece)[NP]) {
    bf16x4 l[NP], h[NP];
    tl_split4<NP>(lo, l);
    tl_split4<NP>(hi, h);
#pragma unroll
    for (int p = 0; p < NP; ++p) piece[p] = __builtin_shufflevector(l[p], h[p], 0, 1, 2, 3, 4, 5, 6, 7);
}

// The products kept of the nine (tests/conv_bounds.py KEPT, tests/conv_pieces.py KEEP; pieces counted from 0 here, so those with
// a + b > NP - 1 are dropped: <= 2^-24 relative at NP = 3): f(a piece, b piece) is called in the order in which every kernel adds
// them to any ONE accumulator -- a3b1, a2b2, a1b3, a2b1, a1b2, a1b1, smallest terms first, so that the small ones meet
// a small sum and are not rounded away against a1b1.  A kernel that loops over its accumulators INSIDE f keeps
// consecutive MFMAs on different accumulators.  The indices are compile-time constants that convert to int, so
// operands indexed by them stay in registers.
template <int NP = 3, class F>
__device__ __forceinline__ void split_products(F&& f) {
    static_assert(NP >= 1 && NP <= 3, "one to three pieces");
    using std::integral_constant;
    if constexpr (NP > 2) {
        f(integral_constant<int, 2>{}, integral_constant<int, 0>{});
        f(integral_constant<int, 1>{}, integral_constant<int, 1>{});
        f(integral_constant<int, 0>{}, integral_constant<int, 2>{});
    }
    if constexpr (NP > 1) {
        f(integral_constant<int, 1>{}, integral_constant<int, 0>{});
        f(integral_constant<int, 0>{}, integral_constant<int, 1>{});
    }
    f(integral_constant<int, 0>{}, integral_constant<int, 0>{});
}

}  // namespace osn
