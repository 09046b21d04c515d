// Regions without a prompt on gfx950: a partition of the voxels of a set of scenes into connected pieces of agreeing
// features, made once and reused for every later prompt (README "Applications": open-vocabulary 3D scene understanding and
// exploration -- "what is in this room?" needs segments before anyone has typed a word).  Single linkage on neighbouring
// voxels: two voxels of the 3^3 self-map are joined iff the dot product of their (unit) feature rows reaches a threshold.
//
//   osn_regions_edges    sim[i, v] = <vox[v], vox[nbr[k_i, v]]> for the offsets below the centre (every undirected edge once)
//   osn_regions_label    union-find (components.h) over the edges with sim >= threshold -> voxel_root[v] = smallest row of v's component
//   osn_regions_records  per region: points, voxels, voxel sums, float box, scene -- integer atomics only
//
// Edges (the hot path).  One wave per voxel.  A row of d fp16 values is d / 8 vectors of 16 bytes; lane l holds vectors
// l and l + 64 (d <= 1024: two at most) of the voxel's own row in registers.  The neighbour rows are wave-uniform, and the
// loads of ALL present neighbours are issued before the first product, so a voxel has up to 13 (26) independent 16-byte
// fetches in flight per lane.  A product of two fp16 values is exact in fp32 (22 significant bits, exponent >= -48), so
// fmaf(a, b, acc) rounds once, at the addition: a lane adds its 8 (16) products in element order, the lanes are added by
// an xor butterfly (32, 16, .. 1): a fixed tree, the same bits on every call.  No LDS, no floating-point atomics.
// The packed fp16 dot instruction is not used: its treatment of fp16 subnormals is not the widening's.  The loads and the
// dot are the body of rowdot.h, which merge.hip runs over an arbitrary pair list.
//
// Label.  voxel_root starts as the identity; one thread per voxel unites it with the earlier neighbours whose sim passes
// (float32 >=: NaN and -inf never pass); a second launch replaces every word by its root.  The root of a tree is its
// smallest row whatever order the hooks landed in (components.h), so the labelling is canonical.
//
// Records.  A lane owns one point; the lanes of a wave that target one region are combined before one lane issues the
// atomics (components.h: wave_combine and BoxVox, with the all-lanes contract and why the records are exact and bitwise
// repeatable).  The box is kept as order-preserving uint32 words in the output arrays and turned into floats by the last
// launch; the region's scene is read at its smallest voxel row.
#include "components.h"
#include "rowdot.h"          // half8, row_load, row_dot

namespace osn {

constexpr int REG_E_NBR = 1, REG_E_INVERSE = 2, REG_E_REGION = 4;
constexpr int REG_T = COMPONENTS_T;
constexpr int REG_WAVES = REG_T / 64;       // voxels of an edge workgroup

// ------------------------------------------------------------------------------------------------------ edges
// NV: 16-byte vectors of a row per lane (1: d <= 512, 2: d <= 1024); NOFF: 13 (connectivity 26) or 3 (6)
template <int NV, int NOFF>
__global__ __launch_bounds__(REG_T) void regions_edges_kernel(const half8* __restrict__ vox, int64_t V, int nvec,
                                                              const int32_t* __restrict__ nbr, float* __restrict__ sim,
                                                              int32_t* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int64_t v = int64_t(blockIdx.x) * REG_WAVES + __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
    if (v >= V) return;                                      // (the whole wave)
    int u[NOFF];
#pragma unroll
    for (int i = 0; i < NOFF; ++i) {
        const int k = NOFF == 13 ? i : face_offset(i);
        int x = __builtin_amdgcn_readfirstlane(nbr[int64_t(k) * V + v]);
        if (x >= V) {                                        // skipped, never dereferenced
            if (lane == 0) atomicOr(err, REG_E_NBR);
            x = -1;
        }
        u[i] = x;
    }
    half8 own[NV], nb[NOFF][NV];
    row_load<NV>(own, vox, int(v), nvec, lane);
#pragma unroll
    for (int i = 0; i < NOFF; ++i) row_load<NV>(nb[i], vox, u[i], nvec, lane);
    float out = 0.f;
#pragma unroll
    for (int i = 0; i < NOFF; ++i) {
        float acc = row_dot<NV>(own, nb[i]);                 // (rowdot.h: the body osn_rows_pair_dot shares)
        if (u[i] < 0) acc = -__builtin_inff();
        if (lane == i) out = acc;
    }
    if (lane < NOFF) sim[int64_t(lane) * V + v] = out;
}

// ------------------------------------------------------------------------------------------------------ label
__global__ __launch_bounds__(REG_T) void regions_init_kernel(int32_t* __restrict__ L, int64_t V) {
    for (int64_t v = int64_t(blockIdx.x) * REG_T + threadIdx.x; v < V; v += int64_t(gridDim.x) * REG_T) L[v] = int32_t(v);
}

__global__ __launch_bounds__(REG_T) void regions_unite_kernel(int32_t* L, const float* __restrict__ sim, const int32_t* __restrict__ nbr,
                                                              int64_t V, int conn, float thr, int32_t* __restrict__ err) {
    const int n_off = conn == 26 ? 13 : 3;
    for (int64_t v = int64_t(blockIdx.x) * REG_T + threadIdx.x; v < V; v += int64_t(gridDim.x) * REG_T) {
        for (int i = 0; i < n_off; ++i) {
            const int k = conn == 26 ? i : face_offset(i);
            const int u = nbr[int64_t(k) * V + v];
            if (u < 0) continue;
            if (u >= V) { atomicOr(err, REG_E_NBR); continue; }
            if (!(sim[int64_t(i) * V + v] >= thr)) continue;  // (NaN and -inf never unite)
            uf_unite(L, int(v), u);
        }
    }
}

__global__ __launch_bounds__(REG_T) void regions_flatten_kernel(int32_t* L, int64_t V) {
    for (int64_t v = int64_t(blockIdx.x) * REG_T + threadIdx.x; v < V; v += int64_t(gridDim.x) * REG_T) uf_flatten(L, int(v));
}

// ------------------------------------------------------------------------------------------------------ records
struct RegOut {
    u64* n_points; u64* n_voxels; u64* vox_sum;              // two's complement int64; vox_sum [R][3]
    uint32_t* box_min; uint32_t* box_max;                    // [R][3]: order-preserving words until the finish launch
    int32_t* scene;                                          // the smallest voxel row until the finish launch
    __device__ BoxArrays box_arrays() const { return {vox_sum, box_min, box_max, 1, 3}; }
};

__global__ __launch_bounds__(REG_T) void regions_preset_kernel(RegOut O, int64_t R) {
    const int64_t r = int64_t(blockIdx.x) * REG_T + threadIdx.x;
    if (r >= R) return;
    O.n_points[r] = 0; O.n_voxels[r] = 0; O.scene[r] = 0x7FFFFFFF;
    BoxVox::preset(O.box_arrays(), r);
}

__global__ __launch_bounds__(REG_T) void regions_voxels_kernel(const int32_t* __restrict__ region, int64_t V, int64_t R, RegOut O,
                                                               int32_t* __restrict__ err) {
    for (int64_t v = int64_t(blockIdx.x) * REG_T + threadIdx.x; v < V; v += int64_t(gridDim.x) * REG_T) {
        const int r = region[v];
        if (r < -1 || r >= R) { atomicOr(err, REG_E_REGION); continue; }
        if (r < 0) continue;
        atomicAdd(&O.n_voxels[r], u64(1));
        atomicMin(&O.scene[r], int32_t(v));
    }
}

__global__ __launch_bounds__(REG_T) void regions_points_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ inv, int64_t n,
                                                               const int4* __restrict__ coords, const int32_t* __restrict__ region,
                                                               int64_t V, int64_t R, RegOut O, int32_t* __restrict__ err) {
    const int64_t p = int64_t(blockIdx.x) * REG_T + threadIdx.x;
    int reg = -1, vx = 0, vy = 0, vz = 0;
    uint32_t bx = 0, by = 0, bz = 0;
    if (p < n) {
        const int v = inv[p];
        if (v < 0 || v >= V) {
            atomicOr(err, REG_E_INVERSE);
        } else {
            const int r = region[v];
            if (r < -1 || r >= R) {
                atomicOr(err, REG_E_REGION);
            } else if (r >= 0) {
                reg = r;
                const int4 cv = coords[v];
                vx = cv.y; vy = cv.z; vz = cv.w;
                bx = f2o(xyz[p * 3 + 0]); by = f2o(xyz[p * 3 + 1]); bz = f2o(xyz[p * 3 + 2]);
            }
        }
    }
    wave_combine<COMBINE_MIN>(reg, BoxVox::point(vx, vy, vz, bx, by, bz), [&](int r, const BoxVox& b, int cnt) {
        atomicAdd(&O.n_points[r], u64(cnt));
        b.commit(O.box_arrays(), r);
    });
}

// words -> floats (a region without points: a zero box); smallest voxel row -> its scene (-1: a region without voxels)
__global__ __launch_bounds__(REG_T) void regions_finish_kernel(RegOut O, int64_t R, const int4* __restrict__ coords, int64_t V) {
    const int64_t r = int64_t(blockIdx.x) * REG_T + threadIdx.x;
    if (r >= R) return;
    const bool some = O.n_points[r] != 0;
    for (int j = 0; j < 3; ++j) {
        const float lo = some ? o2f(O.box_min[r * 3 + j]) : 0.f, hi = some ? o2f(O.box_max[r * 3 + j]) : 0.f;
        O.box_min[r * 3 + j] = __builtin_bit_cast(uint32_t, lo);
        O.box_max[r * 3 + j] = __builtin_bit_cast(uint32_t, hi);
    }
    const int first = O.scene[r];
    O.scene[r] = (first >= 0 && first < V) ? coords[first].x : -1;
}

template <int NV>
static void edges_launch(int conn, dim3 grid, hipStream_t st, const half8* vox, int64_t V, int nvec, const int32_t* nbr, float* sim,
                         int32_t* err) {
    if (conn == 26)
        hipLaunchKernelGGL((regions_edges_kernel<NV, 13>), grid, dim3(REG_T), 0, st, vox, V, nvec, nbr, sim, err);
    else
        hipLaunchKernelGGL((regions_edges_kernel<NV, 3>), grid, dim3(REG_T), 0, st, vox, V, nvec, nbr, sim, err);
}

}  // namespace osn

using namespace osn;

extern "C" int osn_regions_edges(const void* vox_f16, int64_t n_voxels, int d, const int32_t* nbr, int connectivity, float* sim,
                                 int32_t* err, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t V = n_voxels;
    OSN_REQUIRE(V >= 0 && V < (int64_t(1) << 31), OSN_E_ARG, "osn_regions_edges: need 0 <= n_voxels < 2^31 (n_voxels=%lld)", (long long)V);
    OSN_REQUIRE(d >= 8 && d % 8 == 0 && d <= OSN_BANK_POOL_MAX_DIM, OSN_E_ARG, "osn_regions_edges: d=%d (a multiple of 8 in 8 .. %d)", d,
                OSN_BANK_POOL_MAX_DIM);
    OSN_REQUIRE(connectivity == 6 || connectivity == 26, OSN_E_ARG, "osn_regions_edges: connectivity=%d (6 or 26)", connectivity);
    OSN_REQUIRE(err, OSN_E_ARG, "osn_regions_edges: null err");
    if (V == 0) return OSN_OK;
    OSN_REQUIRE(vox_f16 && nbr && sim && aligned16(vox_f16), OSN_E_ARG, "osn_regions_edges: the rows must be non-null and 16-byte aligned");
    const int nvec = d / 8;
    const dim3 grid(unsigned(cdiv(V, REG_WAVES)));
    const half8* vox = static_cast<const half8*>(vox_f16);
    if (nvec <= 64) edges_launch<1>(connectivity, grid, st, vox, V, nvec, nbr, sim, err);
    else edges_launch<2>(connectivity, grid, st, vox, V, nvec, nbr, sim, err);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_regions_label(const float* sim, const int32_t* nbr, int64_t n_voxels, int connectivity, float threshold,
                                 int32_t* voxel_root, int32_t* err, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t V = n_voxels;
    OSN_REQUIRE(V >= 0 && V < (int64_t(1) << 31), OSN_E_ARG, "osn_regions_label: need 0 <= n_voxels < 2^31 (n_voxels=%lld)", (long long)V);
    OSN_REQUIRE(connectivity == 6 || connectivity == 26, OSN_E_ARG, "osn_regions_label: connectivity=%d (6 or 26)", connectivity);
    OSN_REQUIRE(threshold - threshold == 0.0f, OSN_E_ARG, "osn_regions_label: the threshold must be finite");
    OSN_REQUIRE(err, OSN_E_ARG, "osn_regions_label: null err");
    if (V == 0) return OSN_OK;
    OSN_REQUIRE(sim && nbr && voxel_root, OSN_E_ARG, "osn_regions_label: null pointer");
    hipLaunchKernelGGL(regions_init_kernel, dim3(components_grid(V)), dim3(REG_T), 0, st, voxel_root, V);
    hipLaunchKernelGGL(regions_unite_kernel, dim3(components_grid(V)), dim3(REG_T), 0, st, voxel_root, sim, nbr, V, connectivity, threshold, err);
    hipLaunchKernelGGL(regions_flatten_kernel, dim3(components_grid(V)), dim3(REG_T), 0, st, voxel_root, V);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_regions_records(const int32_t* voxel_region, int64_t n_voxels, int64_t n_regions, const float* xyz,
                                   const int32_t* inverse, int64_t n, const int32_t* coords4, int64_t* n_points,
                                   int64_t* n_voxels_out, int64_t* vox_sum, float* box_min, float* box_max, int32_t* scene,
                                   int32_t* err, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t V = n_voxels, R = n_regions;
    OSN_REQUIRE(V >= 0 && V < (int64_t(1) << 31) && n >= 0 && n < (int64_t(1) << 31), OSN_E_ARG,
                "osn_regions_records: need 0 <= n_voxels, n < 2^31 (n_voxels=%lld n=%lld)", (long long)V, (long long)n);
    OSN_REQUIRE(R >= 0 && R <= V, OSN_E_ARG, "osn_regions_records: n_regions=%lld outside [0, n_voxels]", (long long)R);
    OSN_REQUIRE(err, OSN_E_ARG, "osn_regions_records: null err");
    OSN_REQUIRE(V == 0 || (voxel_region && coords4 && aligned16(coords4)), OSN_E_ARG,
                "osn_regions_records: the voxel rows must be non-null and 16-byte aligned");
    OSN_REQUIRE(n == 0 || (xyz && inverse), OSN_E_ARG, "osn_regions_records: null pointer");
    OSN_REQUIRE(R == 0 || (n_points && n_voxels_out && vox_sum && box_min && box_max && scene), OSN_E_ARG, "osn_regions_records: null output");
    RegOut O;
    O.n_points = reinterpret_cast<u64*>(n_points); O.n_voxels = reinterpret_cast<u64*>(n_voxels_out); O.vox_sum = reinterpret_cast<u64*>(vox_sum);
    O.box_min = reinterpret_cast<uint32_t*>(box_min); O.box_max = reinterpret_cast<uint32_t*>(box_max); O.scene = scene;
    const int4* c4 = reinterpret_cast<const int4*>(coords4);
    if (R > 0) hipLaunchKernelGGL(regions_preset_kernel, dim3(unsigned(cdiv(R, REG_T))), dim3(REG_T), 0, st, O, R);
    if (V > 0) hipLaunchKernelGGL(regions_voxels_kernel, dim3(components_grid(V)), dim3(REG_T), 0, st, voxel_region, V, R, O, err);
    if (n > 0) hipLaunchKernelGGL(regions_points_kernel, dim3(unsigned(cdiv(n, REG_T))), dim3(REG_T), 0, st, xyz, inverse, n, c4, voxel_region, V, R, O, err);
    if (R > 0) hipLaunchKernelGGL(regions_finish_kernel, dim3(unsigned(cdiv(R, REG_T))), dim3(REG_T), 0, st, O, R, c4, V);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}
