// The dot product of two fp16 rows by one wave, shared by regions.hip (a voxel with its 3^3 neighbours) and merge.hip (an
// arbitrary pair list): for the same two rows both kernels give the same bits, because both run this body.
//
// A row of d fp16 values is nvec = d / 8 vectors of 16 bytes; lane l holds vectors l and l + 64 (NV = 1: d <= 512, NV = 2:
// d <= 1024), zeros beyond the row.  A product of two fp16 values is exact in fp32 (22 significant bits, exponent >= -48), so
// fmaf(a, b, acc) rounds once, at the addition, and does not depend on which row is a and which is b: a lane adds its 8 (16)
// products in element order, the lanes are added by an xor butterfly (32, 16, .. 1) and every lane receives the sum.  A fixed
// tree: the same bits on every call.  The packed fp16 dot instruction is not used: its treatment of fp16 subnormals is not
// the widening's.  row_dot is called by all 64 lanes of a wave in wave-uniform control flow.
#pragma once
#include "bank.h"            // half8

namespace osn {

// lane's vectors of row `row` (wave-uniform; row < 0: an absent row, which is zeros and is never dereferenced -- the sign test
// sits next to the address so that the compiler forms it with one unsigned 32 x 32 -> 64 bit multiply-add)
template <int NV>
__device__ __forceinline__ void row_load(half8 (&r)[NV], const half8* __restrict__ rows, int row, int nvec, int lane) {
    half8 zero;
#pragma unroll
    for (int c = 0; c < 8; ++c) zero[c] = (_Float16)0.0f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int vec = j * 64 + lane;
        r[j] = (row >= 0 && vec < nvec) ? rows[int64_t(row) * nvec + vec] : zero;
    }
}

template <int NV>
__device__ __forceinline__ float row_dot(const half8 (&a)[NV], const half8 (&b)[NV]) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
#pragma unroll
        for (int c = 0; c < 8; ++c) acc = fmaf(float(a[j][c]), float(b[j][c]), acc);
    }
#pragma unroll
    for (int mk = 32; mk >= 1; mk >>= 1) acc += __shfl_xor(acc, mk, 64);
    return acc;
}

}  // namespace osn
