// What the two connected-component translation units share (objects.hip, regions.hip): the lock-free union-find over one
// 32-bit parent word per element.  Every edge is united once: find both roots, hook the LARGER root under the SMALLER with a
// compare-and-swap, start again from what the CAS returned when it lost.  Parents only ever decrease, a root is the smallest
// row of its tree, and a word that stopped being a root never becomes one again, so whatever order the hooks land in, the
// forest that remains has exactly one root per connected component: the component's smallest row.  Finds read with
// agent-scope loads and halve the path as they go (a stale read only yields an older, still valid, ancestor: the CAS is the
// arbiter).  Also the order-preserving integer image of a float, which both units' records take their boxes through.
#pragma once
#include "common.h"

namespace osn {

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

// order-preserving uint32 of a float (and back)
__device__ inline uint32_t f2o(float f) {
    const uint32_t b = __builtin_bit_cast(uint32_t, f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float o2f(uint32_t o) {
    const uint32_t b = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    return __builtin_bit_cast(float, b);
}

}  // namespace osn
