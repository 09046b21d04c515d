// What the two connected-component translation units share (objects.hip, regions.hip).
//
// Union-find over one 32-bit parent word per element, lock-free.  Every edge is united once: find both roots, hook the
// LARGER root under the SMALLER with a compare-and-swap, start again from what the CAS returned when it lost.  Parents only
// ever decrease, a root is the smallest row of its tree, and a word that stopped being a root never becomes one again, so
// whatever order the hooks land in, the forest that remains has exactly one root per connected component: the component's
// smallest row.  Finds read with agent-scope loads and halve the path as they go (a stale read only yields an older, still
// valid, ancestor: the CAS is the arbiter).
//
// Records.  Every point adds a BoxVox -- its voxel's cell and the order-preserving integer image of its float position --
// to the record of its component: int64 voxel sums, uint32 min / max.  Sums of integers and min / max do not depend on
// order, so the records are exact and the same bits on every call, however the atomics land.  wave_combine merges the
// lanes of a wave that target the same record before ONE lane issues the atomics (a floor puts tens of thousands of
// consecutive points on one record: a dozen same-address atomics per point otherwise).  Its contract:
//   * it is called by ALL 64 LANES of a full wave in wave-uniform control flow (the butterfly reads every lane): the kernels
//     that call it launch COMPONENTS_T-thread workgroups and have no early return, and this must stay so;
//   * a lane outside the group being merged holds identity() -- 0 for a sum, all ones for a min, 0 for a max;
//   * 64 x |coordinate| < 2^21 (coordinates are int16 cells), so the merged voxel sums stay in 32 bits.
#pragma once
#include "common.h"

namespace osn {

typedef unsigned long long u64;

constexpr int COMPONENTS_T = 256;   // threads of a workgroup, both units
constexpr int COMBINE_MIN = 4;      // lanes on one record from which the butterfly beats their own atomics

// blocks of a grid-stride launch over `elems` elements
static inline unsigned components_grid(int64_t elems) {
    const int64_t b = cdiv(elems > 0 ? elems : 1, COMPONENTS_T);
    return unsigned(b < (int64_t(1) << 16) ? b : (int64_t(1) << 16));
}

// offsets below the centre of the 3^3 map, k = ix + 3 iy + 9 iz; the three faces among them: -z = 4, -y = 10, -x = 12
__device__ inline int face_offset(int i) { return i == 0 ? 4 : i == 1 ? 10 : 12; }

// ------------------------------------------------------------------------------------------------------ union-find
__device__ inline int ld_agent(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline int uf_find(int32_t* L, int x) {
    int p = ld_agent(L + x);
    while (p != x) {
        const int g = ld_agent(L + p);                       // g <= p < x
        if (g != p) __hip_atomic_store(L + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // path halving: still an ancestor
        x = p;
        p = g;
    }
    return x;
}

__device__ inline void uf_unite(int32_t* L, int a, int b) {
    while (true) {
        a = uf_find(L, a);
        b = uf_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }        // hook the larger root a under the smaller b
        const int old = atomicCAS(L + a, a, b);
        if (old == a) return;
        a = old;                                             // a had been hooked meanwhile: go on from its parent
    }
}

// after the last unite: the word of element v -> its root
__device__ inline void uf_flatten(int32_t* L, int v) {
    int x = ld_agent(L + v);
    while (true) {                                           // (parents only move towards the root while others flatten)
        const int p = ld_agent(L + x);
        if (p == x) break;
        x = p;
    }
    if (x != v) __hip_atomic_store(L + v, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------------------ records
// order-preserving uint32 of a float (and back)
__device__ inline uint32_t f2o(float f) {
    const uint32_t b = __builtin_bit_cast(uint32_t, f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float o2f(uint32_t o) {
    const uint32_t b = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    return __builtin_bit_cast(float, b);
}

__device__ inline u64 shfl_xor_u64(u64 v, int m) {
    const uint32_t lo = __shfl_xor(uint32_t(v), m, 64), hi = __shfl_xor(uint32_t(v >> 32), m, 64);
    return (u64(hi) << 32) | lo;
}

// where a unit keeps the voxel sums and the box words: component j of record r at [r * record + j * field]
struct BoxArrays {
    u64* vox_sum;                   // two's complement int64
    uint32_t* box_min;
    uint32_t* box_max;
    int64_t field, record;
    __device__ int64_t at(int64_t r, int j) const { return r * record + j * field; }
};

struct BoxVox {
    int v[3];                       // the voxel's cell
    uint32_t lo[3], hi[3];          // f2o of the position
    __device__ static BoxVox identity() { return {{0, 0, 0}, {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, {0u, 0u, 0u}}; }
    __device__ static BoxVox point(int x, int y, int z, uint32_t bx, uint32_t by, uint32_t bz) { return {{x, y, z}, {bx, by, bz}, {bx, by, bz}}; }
    __device__ void merge_xor(int mask) {                    // one butterfly level
#pragma unroll
        for (int j = 0; j < 3; ++j) v[j] += __shfl_xor(v[j], mask, 64);
#pragma unroll
        for (int j = 0; j < 3; ++j) { const uint32_t t = __shfl_xor(lo[j], mask, 64); lo[j] = t < lo[j] ? t : lo[j]; }
#pragma unroll
        for (int j = 0; j < 3; ++j) { const uint32_t t = __shfl_xor(hi[j], mask, 64); hi[j] = t > hi[j] ? t : hi[j]; }
    }
    __device__ void commit(const BoxArrays& A, int64_t r) const {
#pragma unroll
        for (int j = 0; j < 3; ++j) atomicAdd(&A.vox_sum[A.at(r, j)], u64((long long)v[j]));
#pragma unroll
        for (int j = 0; j < 3; ++j) atomicMin(&A.box_min[A.at(r, j)], lo[j]);
#pragma unroll
        for (int j = 0; j < 3; ++j) atomicMax(&A.box_max[A.at(r, j)], hi[j]);
    }
    // the record no point has been added to: what commit() leaves unchanged
    __device__ static void preset(const BoxArrays& A, int64_t r) {
        const BoxVox z = identity();
        for (int j = 0; j < 3; ++j) { A.vox_sum[A.at(r, j)] = u64((long long)z.v[j]); A.box_min[A.at(r, j)] = z.lo[j]; A.box_max[A.at(r, j)] = z.hi[j]; }
    }
};

// One turn per distinct key among the lanes of the wave (key < 0: nothing from this lane).  A group of fewer than MIN lanes:
// each commits its own value, commit(key, value, 1).  Otherwise the others take V::identity(), six levels of V::merge_xor
// run over the whole wave, and the group's first lane commits the merged value with the group's size.  See the contract above.
template <int MIN, class V, class Commit>
__device__ inline void wave_combine(int key, V value, Commit commit) {
    const int lane = threadIdx.x & 63;
    u64 todo = __ballot(key >= 0);
    while (todo) {                                           // (wave-uniform)
        const int leader = __ffsll((long long)todo) - 1;
        const int lk = __shfl(key, leader, 64);
        const bool mine = key == lk;
        const u64 m = __ballot(mine);
        todo &= ~m;
        const int cnt = __popcll(m);
        if (cnt < MIN) {
            if (mine) commit(key, value, 1);
            continue;
        }
        V a = mine ? value : V::identity();
#pragma unroll
        for (int mk = 32; mk >= 1; mk >>= 1) a.merge_xor(mk);
        if (lane == leader) commit(lk, a, cnt);
    }
}

}  // namespace osn
