// Merge regions by mean feature on gfx950: the second stage after the single-linkage regions of regions.hip.  Over-segment,
// then unite ADJACENT regions whose mean features agree: the mean of a grown region does not drift along a chain of pairwise
// similar voxels the way single linkage does.  The loop lives in openscene_amd/merge.py; the kernels of one round are here.
//
//   osn_merge_contacts   key[i, v] = (lo << 32 | hi) of the regions of voxel v and its neighbour below the centre, or -1
//   osn_rows_pair_dot    sim[e] = <rows[lo[e]], rows[hi[e]]> over an arbitrary pair list (the hot path)
//   osn_merge_round      best neighbour per region by a 64-bit atomic maximum, star contraction, union-find -> parent
//   osn_rows_fold        the float32 sums of the merged groups, row after row in list order
//
// Pair dot.  A wave takes MERGE_RUN consecutive pairs; the pair indices are wave-uniform (scalar loads, scalar compares).  The
// loads of ALL rows of the run are issued before the first product, as the edge kernel does for its 13 neighbours; the list
// is sorted by (lo, hi), so consecutive pairs mostly share their lo row, which is then kept in registers and not loaded
// again.  A region with thousands of neighbours is thousands of pairs cut into runs like any others.  The arithmetic is the
// body of rowdot.h, the one regions_edges_kernel runs: the same bits for the same two rows.  No LDS, no floating-point
// atomics.
//
// Round.  An edge e with sim[e] >= threshold (float32: NaN and -inf never pass) has the key
// (f2o(sim[e]) << 32) | (0xFFFFFFFF - e): greater similarity wins, then the lower edge index; -0 orders below +0 (f2o).
// e < 2^32 - 1 keeps every key above 0, the preset "no eligible edge".  best[a] is the atomic maximum over a's eligible
// edges -- a maximum of integers does not depend on the order the atomics land in.  An edge is mutual when both ends name it
// as their best.  Region a with best edge (a, b) is united with b iff that edge is mutual or b's best edge is mutual: a mutual
// pair and the regions that point at it (a star), never a whole best-neighbour tree, which would be single linkage again.
// The unions go through uf_unite / uf_flatten (components.h), so parent[a] is the smallest member of a's group whatever
// the scheduling.  The globally greatest key is mutual, so a round with an eligible edge merges something.
//
// Fold.  Lane l of a wave owns four columns of one group and adds the group's rows one after the other, starting from +0,
// in list order, sixteen loads in flight: no atomics, the bits are a function of the inputs.
#include "components.h"
#include "rowdot.h"

namespace osn {

constexpr int REG_E_NBR = 1, REG_E_REGION = 4, REG_E_PAIR = 8;      // bits 1, 2, 4: regions.hip
constexpr int MRG_T = COMPONENTS_T;
constexpr int MRG_WAVES = MRG_T / 64;
constexpr int MERGE_RUN = 8;                // pairs of a wave (chosen from the register counts of both widths)
constexpr int FOLD_FLIGHT = 16;             // rows of a group loaded before they are added

// ------------------------------------------------------------------------------------------------------ contacts
__global__ __launch_bounds__(MRG_T) void merge_contacts_kernel(const int32_t* __restrict__ region, const int32_t* __restrict__ nbr,
                                                               int64_t V, int conn, int64_t R, long long* __restrict__ key,
                                                               int32_t* __restrict__ err) {
    const int n_off = conn == 26 ? 13 : 3;
    for (int64_t v = int64_t(blockIdx.x) * MRG_T + threadIdx.x; v < V; v += int64_t(gridDim.x) * MRG_T) {
        const int ra = region[v];
        const bool bad_a = ra < -1 || ra >= R;
        if (bad_a) atomicOr(err, REG_E_REGION);
        for (int i = 0; i < n_off; ++i) {
            const int k = conn == 26 ? i : face_offset(i);
            const int u = nbr[int64_t(k) * V + v];
            long long out = -1;
            if (u >= V) {
                atomicOr(err, REG_E_NBR);                    // skipped, never dereferenced
            } else if (u >= 0) {
                const int rb = region[u];
                if (rb < -1 || rb >= R) {
                    atomicOr(err, REG_E_REGION);
                } else if (!bad_a && ra >= 0 && rb >= 0 && ra != rb) {
                    const int lo = ra < rb ? ra : rb, hi = ra < rb ? rb : ra;
                    out = (long long)((u64(uint32_t(lo)) << 32) | uint32_t(hi));
                }
            }
            key[int64_t(i) * V + v] = out;
        }
    }
}

// ------------------------------------------------------------------------------------------------------ pair dot
// NV: 16-byte vectors of a row per lane (1: d <= 512, 2: d <= 1024)
template <int NV>
__global__ __launch_bounds__(MRG_T) void rows_pair_dot_kernel(const half8* __restrict__ rows, int64_t R, int nvec,
                                                              const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, int64_t E,
                                                              float* __restrict__ sim, int32_t* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int64_t e0 = (int64_t(blockIdx.x) * MRG_WAVES + __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6))) * MERGE_RUN;
    if (e0 >= E) return;                                     // (the whole wave)
    int a[MERGE_RUN], b[MERGE_RUN];                          // -1: no pair here; -2: an end out of range
    bool bad = false;
#pragma unroll
    for (int i = 0; i < MERGE_RUN; ++i) {
        a[i] = b[i] = -1;
        if (e0 + i < E) {
            a[i] = __builtin_amdgcn_readfirstlane(lo[e0 + i]);
            b[i] = __builtin_amdgcn_readfirstlane(hi[e0 + i]);
            if (a[i] < 0 || a[i] >= R || b[i] < 0 || b[i] >= R) {     // skipped, never dereferenced
                a[i] = b[i] = -2;
                bad = true;
            }
        }
    }
    if (bad && lane == 0) atomicOr(err, REG_E_PAIR);
    half8 ra[MERGE_RUN][NV], rb[MERGE_RUN][NV];
#pragma unroll
    for (int i = 0; i < MERGE_RUN; ++i) {
        if (i > 0 && a[i] >= 0 && a[i] == a[i - 1]) {        // (wave-uniform) the lo row is kept while the pairs share it
#pragma unroll
            for (int j = 0; j < NV; ++j) ra[i][j] = ra[i - 1][j];
        } else {
            row_load<NV>(ra[i], rows, a[i], nvec, lane);
        }
        row_load<NV>(rb[i], rows, b[i], nvec, lane);
    }
    float out = 0.f;
#pragma unroll
    for (int i = 0; i < MERGE_RUN; ++i) {
        float acc = row_dot<NV>(ra[i], rb[i]);
        if (a[i] < 0) acc = -__builtin_inff();
        if (lane == i) out = acc;
    }
    if (lane < MERGE_RUN && e0 + lane < E) sim[e0 + lane] = out;
}

// ------------------------------------------------------------------------------------------------------ round
__global__ __launch_bounds__(MRG_T) void merge_preset_kernel(u64* __restrict__ best, int32_t* __restrict__ parent, int64_t R) {
    for (int64_t r = int64_t(blockIdx.x) * MRG_T + threadIdx.x; r < R; r += int64_t(gridDim.x) * MRG_T) {
        best[r] = 0;
        parent[r] = int32_t(r);
    }
}

__device__ inline bool pair_ok(int a, int b, int64_t R) { return a >= 0 && a < R && b >= 0 && b < R; }

__global__ __launch_bounds__(MRG_T) void merge_best_kernel(const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                           const float* __restrict__ sim, int64_t E, int64_t R, float thr,
                                                           u64* __restrict__ best, int32_t* __restrict__ err) {
    for (int64_t e = int64_t(blockIdx.x) * MRG_T + threadIdx.x; e < E; e += int64_t(gridDim.x) * MRG_T) {
        const int a = lo[e], b = hi[e];
        if (!pair_ok(a, b, R)) { atomicOr(err, REG_E_PAIR); continue; }
        if (a == b) continue;                                // (a pair of one region with itself says nothing)
        const float s = sim[e];
        if (!(s >= thr)) continue;                           // (NaN and -inf never pass)
        const u64 k = (u64(f2o(s)) << 32) | u64(0xFFFFFFFFu - uint32_t(e));
        atomicMax(best + a, k);
        atomicMax(best + b, k);
    }
}

// the other end of the edge a key names, seen from region x (the key was written by a valid edge with x as one end)
__device__ inline int key_other(u64 k, int x, const int32_t* __restrict__ lo, const int32_t* __restrict__ hi) {
    const int64_t e = int64_t(0xFFFFFFFFu - uint32_t(k));
    const int a = lo[e];
    return a == x ? hi[e] : a;
}

__global__ __launch_bounds__(MRG_T) void merge_unite_kernel(const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                            const u64* __restrict__ best, int64_t R, int32_t* parent) {
    for (int64_t r = int64_t(blockIdx.x) * MRG_T + threadIdx.x; r < R; r += int64_t(gridDim.x) * MRG_T) {
        const int a = int(r);
        const u64 ka = best[a];
        if (ka == 0) continue;
        const int b = key_other(ka, a, lo, hi);
        const u64 kb = best[b];                              // (not 0: b is an end of the eligible edge ka)
        bool take = kb == ka;                                // mutual
        if (!take) take = best[key_other(kb, b, lo, hi)] == kb;          // b's best edge is mutual: a joins the star
        if (take) uf_unite(parent, a, b);
    }
}

__global__ __launch_bounds__(MRG_T) void merge_flatten_kernel(int32_t* parent, int64_t R) {
    for (int64_t r = int64_t(blockIdx.x) * MRG_T + threadIdx.x; r < R; r += int64_t(gridDim.x) * MRG_T) uf_flatten(parent, int(r));
}

// ------------------------------------------------------------------------------------------------------ fold
__global__ __launch_bounds__(MRG_T) void rows_fold_kernel(const float4* __restrict__ src, int64_t R_old, int nq,
                                                          const int64_t* __restrict__ starts, const int32_t* __restrict__ members,
                                                          int64_t L, int64_t G, float4* __restrict__ dst, int32_t* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int64_t g = int64_t(blockIdx.x) * MRG_WAVES + __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
    const int q = blockIdx.y * 64 + lane;                    // the lane's four columns
    if (g >= G) return;                                      // (the whole wave)
    int64_t a = starts[g], b = starts[g + 1];
    if (a < 0 || b < a || b > L) {                           // clamped: nothing is read out of bounds whatever starts holds
        if (lane == 0 && blockIdx.y == 0) atomicOr(err, REG_E_REGION);
        a = a < 0 ? 0 : (a > L ? L : a);
        b = b < a ? a : (b > L ? L : b);
    }
    // members of the batch at i (wave-uniform); -1: past the group, or out of range (skipped, never dereferenced)
    auto batch = [&](int64_t i, int (&m)[FOLD_FLIGHT]) {
#pragma unroll
        for (int j = 0; j < FOLD_FLIGHT; ++j) {
            m[j] = -1;
            if (i + j < b) {
                m[j] = __builtin_amdgcn_readfirstlane(members[i + j]);
                if (m[j] < 0 || m[j] >= R_old) {
                    if (lane == 0 && blockIdx.y == 0) atomicOr(err, REG_E_REGION);
                    m[j] = -1;
                }
            }
        }
    };
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int m[FOLD_FLIGHT], next[FOLD_FLIGHT];
    batch(a, m);
    for (int64_t i = a; i < b; i += FOLD_FLIGHT) {
        float4 x[FOLD_FLIGHT];
#pragma unroll
        for (int j = 0; j < FOLD_FLIGHT; ++j)
            x[j] = (m[j] >= 0 && q < nq) ? src[int64_t(m[j]) * nq + q] : make_float4(0.f, 0.f, 0.f, 0.f);
        batch(i + FOLD_FLIGHT, next);                        // the next batch's indices travel under this batch's rows
#pragma unroll
        for (int j = 0; j < FOLD_FLIGHT; ++j) {              // list order, one row after the other
            if (m[j] >= 0) { acc.x += x[j].x; acc.y += x[j].y; acc.z += x[j].z; acc.w += x[j].w; }
            m[j] = next[j];
        }
    }
    if (q < nq) dst[g * nq + q] = acc;
}

}  // namespace osn

using namespace osn;

extern "C" int osn_merge_contacts(const int32_t* voxel_region, const int32_t* nbr, int64_t n_voxels, int connectivity,
                                  int64_t n_regions, int64_t* key, int32_t* err, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t V = n_voxels, R = n_regions;
    OSN_REQUIRE(V >= 0 && V < (int64_t(1) << 31), OSN_E_ARG, "osn_merge_contacts: need 0 <= n_voxels < 2^31 (n_voxels=%lld)", (long long)V);
    OSN_REQUIRE(R >= 0 && R <= V, OSN_E_ARG, "osn_merge_contacts: n_regions=%lld outside [0, n_voxels]", (long long)R);
    OSN_REQUIRE(connectivity == 6 || connectivity == 26, OSN_E_ARG, "osn_merge_contacts: connectivity=%d (6 or 26)", connectivity);
    OSN_REQUIRE(err, OSN_E_ARG, "osn_merge_contacts: null err");
    if (V == 0) return OSN_OK;
    OSN_REQUIRE(voxel_region && nbr && key, OSN_E_ARG, "osn_merge_contacts: null pointer");
    hipLaunchKernelGGL(merge_contacts_kernel, dim3(components_grid(V)), dim3(MRG_T), 0, st, voxel_region, nbr, V, connectivity, R,
                       reinterpret_cast<long long*>(key), err);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_rows_pair_dot(const void* rows_f16, int64_t n_rows, int d, const int32_t* lo, const int32_t* hi, int64_t n_pairs,
                                 float* sim, int32_t* err, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t R = n_rows, E = n_pairs;
    OSN_REQUIRE(R >= 0 && R < (int64_t(1) << 31), OSN_E_ARG, "osn_rows_pair_dot: need 0 <= n_rows < 2^31 (n_rows=%lld)", (long long)R);
    OSN_REQUIRE(E >= 0 && E < (int64_t(1) << 32) - 1, OSN_E_ARG, "osn_rows_pair_dot: need 0 <= n_pairs < 2^32 - 1 (n_pairs=%lld)", (long long)E);
    OSN_REQUIRE(d >= 8 && d % 8 == 0 && d <= OSN_BANK_POOL_MAX_DIM, OSN_E_ARG, "osn_rows_pair_dot: d=%d (a multiple of 8 in 8 .. %d)", d,
                OSN_BANK_POOL_MAX_DIM);
    OSN_REQUIRE(err, OSN_E_ARG, "osn_rows_pair_dot: null err");
    if (E == 0) return OSN_OK;
    OSN_REQUIRE(lo && hi && sim, OSN_E_ARG, "osn_rows_pair_dot: null pointer");
    OSN_REQUIRE(R == 0 || (rows_f16 && aligned16(rows_f16)), OSN_E_ARG, "osn_rows_pair_dot: the rows must be non-null and 16-byte aligned");
    const int nvec = d / 8;
    const dim3 grid(unsigned(cdiv(E, int64_t(MRG_WAVES) * MERGE_RUN)));
    const half8* rows = static_cast<const half8*>(rows_f16);
    if (nvec <= 64) hipLaunchKernelGGL((rows_pair_dot_kernel<1>), grid, dim3(MRG_T), 0, st, rows, R, nvec, lo, hi, E, sim, err);
    else hipLaunchKernelGGL((rows_pair_dot_kernel<2>), grid, dim3(MRG_T), 0, st, rows, R, nvec, lo, hi, E, sim, err);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" size_t osn_merge_ws_bytes(int64_t n_regions) { return size_t(n_regions > 0 ? n_regions : 0) * sizeof(u64); }

extern "C" int osn_merge_round(const int32_t* lo, const int32_t* hi, const float* sim, int64_t n_pairs, int64_t n_regions,
                               float threshold, int32_t* parent, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t E = n_pairs, R = n_regions;
    OSN_REQUIRE(R >= 0 && R < (int64_t(1) << 31), OSN_E_ARG, "osn_merge_round: need 0 <= n_regions < 2^31 (n_regions=%lld)", (long long)R);
    OSN_REQUIRE(E >= 0 && E < (int64_t(1) << 32) - 1, OSN_E_ARG, "osn_merge_round: need 0 <= n_pairs < 2^32 - 1 (n_pairs=%lld)", (long long)E);
    OSN_REQUIRE(threshold - threshold == 0.0f, OSN_E_ARG, "osn_merge_round: the threshold must be finite");
    OSN_REQUIRE(err, OSN_E_ARG, "osn_merge_round: null err");
    if (R == 0) return OSN_OK;
    OSN_REQUIRE(parent, OSN_E_ARG, "osn_merge_round: null parent");
    OSN_REQUIRE(E == 0 || (lo && hi && sim), OSN_E_ARG, "osn_merge_round: null pointer");
    OSN_REQUIRE(ws && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0 && ws_bytes >= osn_merge_ws_bytes(R), OSN_E_ARG,
                "osn_merge_round: the workspace must be 8-byte aligned and hold osn_merge_ws_bytes(n_regions) = %zu bytes (got %zu)",
                osn_merge_ws_bytes(R), ws_bytes);
    u64* best = static_cast<u64*>(ws);
    hipLaunchKernelGGL(merge_preset_kernel, dim3(components_grid(R)), dim3(MRG_T), 0, st, best, parent, R);
    if (E > 0) {
        hipLaunchKernelGGL(merge_best_kernel, dim3(components_grid(E)), dim3(MRG_T), 0, st, lo, hi, sim, E, R, threshold, best, err);
        hipLaunchKernelGGL(merge_unite_kernel, dim3(components_grid(R)), dim3(MRG_T), 0, st, lo, hi, best, R, parent);
        hipLaunchKernelGGL(merge_flatten_kernel, dim3(components_grid(R)), dim3(MRG_T), 0, st, parent, R);
    }
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_rows_fold(const float* src, int64_t n_src, int d, const int64_t* starts, const int32_t* members, int64_t n_members,
                             int64_t n_groups, float* dst, int32_t* err, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t G = n_groups, L = n_members, R = n_src;
    OSN_REQUIRE(R >= 0 && R < (int64_t(1) << 31) && G >= 0 && G < (int64_t(1) << 31) && L >= 0, OSN_E_ARG,
                "osn_rows_fold: need 0 <= n_src, n_groups < 2^31 and n_members >= 0 (n_src=%lld n_groups=%lld n_members=%lld)", (long long)R,
                (long long)G, (long long)L);
    OSN_REQUIRE(d >= 8 && d % 8 == 0 && d <= OSN_BANK_POOL_MAX_DIM, OSN_E_ARG, "osn_rows_fold: d=%d (a multiple of 8 in 8 .. %d)", d,
                OSN_BANK_POOL_MAX_DIM);
    OSN_REQUIRE(err, OSN_E_ARG, "osn_rows_fold: null err");
    if (G == 0) return OSN_OK;
    OSN_REQUIRE(starts && dst && aligned16(dst), OSN_E_ARG, "osn_rows_fold: starts and dst must be non-null, dst 16-byte aligned");
    OSN_REQUIRE(L == 0 || members, OSN_E_ARG, "osn_rows_fold: null members");
    OSN_REQUIRE(R == 0 || (src && aligned16(src)), OSN_E_ARG, "osn_rows_fold: src must be non-null and 16-byte aligned");
    const int nq = d / 4;
    const dim3 grid(unsigned(cdiv(G, MRG_WAVES)), unsigned(cdiv(nq, 64)));
    hipLaunchKernelGGL(rows_fold_kernel, grid, dim3(MRG_T), 0, st, reinterpret_cast<const float4*>(src), R, nq, starts, members, L, G,
                       reinterpret_cast<float4*>(dst), err);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}
