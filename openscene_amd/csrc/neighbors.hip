// Spatial neighbours on the voxel grid on gfx950: the k nearest source points of a query inside the 27 cells around it, and
// the two gathers that move a per-point result (a heat-map, a feature matrix, labels) along the neighbour lists -- to other
// point sets, into the rows feature fusion never saw (run/evaluate.py:297-300: "some points do not have 2D features from 2D
// feature fusion"), or over a point's surroundings before a threshold.
//
//   osn_knn_grid    per query the k smallest keys (bits of float32 d2 << 32 | point index) over the source points of the
//                   27 cells nbr[., q_cell]; d2 <= r2 only; -> idx, dist2, count
//   osn_knn_blend   out[m] = sum_j w_j values[idx[m, j]] / sum_j w_j in ascending j, fp32, rounded once to the values' type
//   osn_knn_vote    the label most of a query's neighbours hold; ties go to the label whose first holder is nearest
//
// Search.  d2 >= 0, so its bits order as an unsigned integer and ONE 64-bit key carries the whole order (d2, then point
// index), as the z-buffer key of render.hip does.  d2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)) from separately rounded
// float32 operations (contraction into FMA is switched off for the file): numpy float32 gives the same bits.  The
// candidates are a set and the result is its k smallest keys: a pure function of the inputs, whatever the schedule.
//
// Work layout.  One lane per query; the k best keys are a sorted list of 64-bit registers, fully unrolled (instances for k
// rounded up to 1, 4, 8, 16; none uses scratch).  A new key is compared with the worst kept one first, so the insertion
// network runs only for a candidate that enters the list.  The queries are taken in the order the caller gives -- cell
// order -- so the lanes of a wave walk the same 27 point lists: their loads hit the same lines and their loops have the same
// trip counts.  A cell's list is walked four candidates at a time: four indices, then four points, are in flight before the
// first distance.  The results go to the query's own row.
//
// Every index read from memory is checked before it is used: an order entry against M, a cell column against the table, a
// table entry against V, a list range against n_src, a point against N, a neighbour against N.  A bad entry is skipped and
// recorded in the err word; the wrapper raises on it.  No floating-point atomics, no LDS.
#include "common.h"
#include <hip/hip_fp16.h>

// Every float32 operation of this file rounds on its own.  The operators are written plainly under this pragma: the
// __fmul_rn / __fadd_rn intrinsics are operators inside a header, compiled under the default, which contracts them into FMA.
#pragma clang fp contract(off)

namespace osn {

using u64 = unsigned long long;
constexpr int KNN_T = 256;
constexpr int KNN_MAX_K = 16;
constexpr int KNN_E_ORDER = 1, KNN_E_CELL = 2, KNN_E_POINT = 4, KNN_E_NEIGHBOR = 8;
constexpr u64 KNN_NONE = ~u64(0);

template <int KK>
struct Best {
    u64 key[KK];                                             // ascending
    __device__ void init() {
#pragma unroll
        for (int i = 0; i < KK; ++i) key[i] = KNN_NONE;
    }
    __device__ void push(u64 x) {
        if (x < key[KK - 1]) {
            key[KK - 1] = x;
#pragma unroll
            for (int i = KK - 1; i > 0; --i) {
                const u64 a = key[i - 1], b = key[i];
                const bool sw = b < a;
                key[i - 1] = sw ? b : a;
                key[i] = sw ? a : b;
            }
        }
    }
};

struct KnnArgs {
    const float* xyz; int64_t n;
    const int32_t* cell_start; const int32_t* cell_points; int64_t n_src, n_voxels;
    const int32_t* nbr; int64_t n_cells;
    const float* query; const int32_t* q_cell; const int32_t* exclude; const int32_t* order; int64_t m;
    int k; float r2;
    int32_t* idx; float* dist2; int32_t* count; int32_t* err;
};

template <int KK>
__global__ __launch_bounds__(KNN_T) void knn_grid_kernel(KnnArgs a) {
    const int64_t t = int64_t(blockIdx.x) * KNN_T + threadIdx.x;
    if (t >= a.m) return;
    int64_t q = t;
    if (a.order) {
        q = a.order[t];
        if (q < 0 || q >= a.m) { atomicOr(a.err, KNN_E_ORDER); return; }
    }
    int64_t c = a.q_cell[q];
    if (c < -1 || c >= a.n_cells) { atomicOr(a.err, KNN_E_CELL); c = -1; }
    Best<KK> best;
    best.init();
    if (c >= 0) {
        const float qx = a.query[q * 3 + 0], qy = a.query[q * 3 + 1], qz = a.query[q * 3 + 2];
        const int ex = a.exclude ? a.exclude[q] : -1;
        for (int o = 0; o < 27; ++o) {
            const int64_t v = a.nbr[int64_t(o) * a.n_cells + c];
            if (v < 0) continue;
            if (v >= a.n_voxels) { atomicOr(a.err, KNN_E_CELL); continue; }
            const int64_t s = a.cell_start[v], e = a.cell_start[v + 1];
            if (s < 0 || e > a.n_src || s > e) { atomicOr(a.err, KNN_E_POINT); continue; }
            for (int64_t j = s; j < e; j += 4) {
                int p[4];
                float px[4], py[4], pz[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) p[u] = j + u < e ? a.cell_points[j + u] : -1;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (j + u < e && (p[u] < 0 || p[u] >= a.n)) { atomicOr(a.err, KNN_E_POINT); p[u] = -1; }
                    if (p[u] == ex) p[u] = -1;
                    px[u] = py[u] = pz[u] = 0.f;
                    if (p[u] >= 0) {
                        const float* s3 = a.xyz + int64_t(p[u]) * 3;
                        px[u] = s3[0]; py[u] = s3[1]; pz[u] = s3[2];
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (p[u] < 0) continue;
                    const float dx = qx - px[u], dy = qy - py[u], dz = qz - pz[u];
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    if (d2 <= a.r2) best.push((u64(__float_as_uint(d2)) << 32) | u64(uint32_t(p[u])));      // (NaN fails)
                }
            }
        }
    }
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < KK; ++j) {
        if (j < a.k) {
            const u64 key = best.key[j];
            const bool some = key != KNN_NONE;
            cnt += some ? 1 : 0;
            a.idx[q * a.k + j] = some ? int32_t(uint32_t(key)) : -1;
            a.dist2[q * a.k + j] = some ? __uint_as_float(uint32_t(key >> 32)) : __builtin_inff();
        }
    }
    a.count[q] = cnt;
}

// ------------------------------------------------------------------------------------------------------ blend
template <typename T, int VEC>
struct alignas(sizeof(T) * VEC) Pack {
    T v[VEC];
};

__device__ inline float to_float(float x) { return x; }
__device__ inline float to_float(__half x) { return __half2float(x); }
template <typename T> __device__ inline T from_float(float x);
template <> __device__ inline float from_float<float>(float x) { return x; }
template <> __device__ inline __half from_float<__half>(float x) { return __float2half_rn(x); }

// Lanes run along the row in units of VEC values; a query is served by a group of `1 << shift` lanes (the row's units rounded
// up to a power of two, 64 at most), so a wave holds 64 >> shift queries: a one-column heat-map keeps all 64 lanes busy.
// All (at most KK: k rounded up to 1, 4, 8 or 16) neighbour rows of a unit are loaded before the first product; a small k
// holds few registers, so more waves are resident to keep loads in flight.
template <typename T, int VEC, int KK>
__global__ __launch_bounds__(KNN_T) void knn_blend_kernel(const T* __restrict__ values, int64_t n, int64_t C, int units,
                                                          const int32_t* __restrict__ idx, const float* __restrict__ dist2,
                                                          const int32_t* __restrict__ count, int64_t m, int k, int inverse, float eps,
                                                          float fill, T* __restrict__ out, uint8_t* __restrict__ found,
                                                          int32_t* __restrict__ err, int shift) {
    const int64_t t = int64_t(blockIdx.x) * KNN_T + threadIdx.x;
    const int64_t g = t >> shift;
    const int width = 1 << shift, l = int(t) & (width - 1);
    if (g >= m) return;
    int cnt = count[g];
    if (cnt < 0 || cnt > k) { atomicOr(err, KNN_E_NEIGHBOR); cnt = cnt < 0 ? 0 : k; }
    int nb[KK];
    float w[KK];
    float den = 0.f;
    bool any = false;
#pragma unroll
    for (int j = 0; j < KK; ++j) {
        nb[j] = -1;
        w[j] = 0.f;
        if (j < cnt) {
            int p = idx[g * k + j];
            if (p < 0 || p >= n) { atomicOr(err, KNN_E_NEIGHBOR); p = -1; }
            nb[j] = p;
            if (p >= 0) {
                w[j] = inverse ? 1.f / (dist2[g * k + j] + eps) : 1.f;
                den = any ? den + w[j] : w[j];
                any = true;
            }
        }
    }
    if (l == 0) found[g] = any ? 1 : 0;
    const T fill_t = from_float<T>(fill);
    for (int u = l; u < units; u += width) {
        Pack<T, VEC> r[KK], o;
#pragma unroll
        for (int j = 0; j < KK; ++j)
            if (nb[j] >= 0) r[j] = *reinterpret_cast<const Pack<T, VEC>*>(values + int64_t(nb[j]) * C + int64_t(u) * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            float num = 0.f;
            bool first = true;
#pragma unroll
            for (int j = 0; j < KK; ++j) {
                if (nb[j] >= 0) {
                    const float prod = w[j] * to_float(r[j].v[e]);
                    num = first ? prod : num + prod;               // (the sum starts AT the first product: -0 stays -0)
                    first = false;
                }
            }
            o.v[e] = any ? from_float<T>(num / den) : fill_t;
        }
        *reinterpret_cast<Pack<T, VEC>*>(out + g * C + int64_t(u) * VEC) = o;
    }
}

// ------------------------------------------------------------------------------------------------------ vote
__global__ __launch_bounds__(KNN_T) void knn_vote_kernel(const int64_t* __restrict__ labels, int64_t n, const int32_t* __restrict__ idx,
                                                         const int32_t* __restrict__ count, int64_t m, int k, int64_t fill,
                                                         int64_t* __restrict__ out, int32_t* __restrict__ err) {
    const int64_t g = int64_t(blockIdx.x) * KNN_T + threadIdx.x;
    if (g >= m) return;
    int cnt = count[g];
    if (cnt < 0 || cnt > k) { atomicOr(err, KNN_E_NEIGHBOR); cnt = cnt < 0 ? 0 : k; }
    int64_t lab[KNN_MAX_K];
#pragma unroll
    for (int j = 0; j < KNN_MAX_K; ++j) {
        lab[j] = -1;
        if (j < cnt) {
            const int p = idx[g * k + j];
            if (p < 0 || p >= n) atomicOr(err, KNN_E_NEIGHBOR);
            else lab[j] = labels[p];
        }
    }
    int64_t win = fill;
    int most = 0;
#pragma unroll
    for (int j = 0; j < KNN_MAX_K; ++j) {
        int votes = 0;
#pragma unroll
        for (int i = 0; i < KNN_MAX_K; ++i) votes += lab[i] == lab[j] ? 1 : 0;
        if (lab[j] >= 0 && votes > most) { most = votes; win = lab[j]; }      // (strictly more: a tie stays with the smaller j)
    }
    out[g] = win;
}

template <typename T, int VEC>
static void blend_launch(hipStream_t st, const void* values, int64_t n, int64_t C, const int32_t* idx, const float* dist2,
                         const int32_t* count, int64_t m, int k, int inverse, float eps, float fill, void* out, uint8_t* found,
                         int32_t* err) {
    const int units = int(C / VEC);
    int shift = 0;
    while ((1 << shift) < units && shift < 6) ++shift;
    const int64_t threads = m << shift;
    const dim3 grid(unsigned(cdiv(threads, KNN_T))), block(KNN_T);
    const T* v = static_cast<const T*>(values);
    T* o = static_cast<T*>(out);
    if (k == 1) hipLaunchKernelGGL((knn_blend_kernel<T, VEC, 1>), grid, block, 0, st, v, n, C, units, idx, dist2, count, m, k, inverse, eps, fill, o, found, err, shift);
    else if (k <= 4) hipLaunchKernelGGL((knn_blend_kernel<T, VEC, 4>), grid, block, 0, st, v, n, C, units, idx, dist2, count, m, k, inverse, eps, fill, o, found, err, shift);
    else if (k <= 8) hipLaunchKernelGGL((knn_blend_kernel<T, VEC, 8>), grid, block, 0, st, v, n, C, units, idx, dist2, count, m, k, inverse, eps, fill, o, found, err, shift);
    else hipLaunchKernelGGL((knn_blend_kernel<T, VEC, 16>), grid, block, 0, st, v, n, C, units, idx, dist2, count, m, k, inverse, eps, fill, o, found, err, shift);
}

}  // namespace osn

using namespace osn;

extern "C" int osn_knn_grid(const float* xyz, int64_t n, const int32_t* cell_start, const int32_t* cell_points, int64_t n_src,
                            int64_t n_voxels, const int32_t* nbr, int64_t n_cells, const float* query_xyz, const int32_t* q_cell,
                            const int32_t* exclude, const int32_t* order, int64_t m, int k, float r2, int32_t* idx, float* dist2,
                            int32_t* count, int32_t* err, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t lim = int64_t(1) << 31;
    OSN_REQUIRE(n >= 0 && n < lim && m >= 0 && m < lim / KNN_MAX_K && n_voxels >= 0 && n_voxels < lim && n_cells >= 0 && n_cells < lim / 27,
                OSN_E_ARG, "osn_knn_grid: sizes out of range (n=%lld m=%lld n_voxels=%lld n_cells=%lld)", (long long)n, (long long)m,
                (long long)n_voxels, (long long)n_cells);
    OSN_REQUIRE(n_src >= 0 && n_src <= n, OSN_E_ARG, "osn_knn_grid: n_src=%lld outside [0, n]", (long long)n_src);
    OSN_REQUIRE(k >= 1 && k <= KNN_MAX_K, OSN_E_ARG, "osn_knn_grid: k=%d outside 1 .. %d", k, KNN_MAX_K);
    OSN_REQUIRE(r2 >= 0.f && r2 - r2 == 0.f, OSN_E_ARG, "osn_knn_grid: r2 must be finite and >= 0");
    OSN_REQUIRE(err, OSN_E_ARG, "osn_knn_grid: null err");
    if (m == 0) return OSN_OK;
    OSN_REQUIRE(query_xyz && q_cell && idx && dist2 && count && cell_start, OSN_E_ARG, "osn_knn_grid: null pointer");
    OSN_REQUIRE((n == 0 || xyz) && (n_src == 0 || cell_points) && (n_cells == 0 || nbr), OSN_E_ARG, "osn_knn_grid: null pointer");
    KnnArgs a;
    a.xyz = xyz; a.n = n; a.cell_start = cell_start; a.cell_points = cell_points; a.n_src = n_src; a.n_voxels = n_voxels;
    a.nbr = nbr; a.n_cells = n_cells; a.query = query_xyz; a.q_cell = q_cell; a.exclude = exclude; a.order = order; a.m = m;
    a.k = k; a.r2 = r2; a.idx = idx; a.dist2 = dist2; a.count = count; a.err = err;
    const dim3 grid(unsigned(cdiv(m, KNN_T))), block(KNN_T);
    if (k == 1) hipLaunchKernelGGL(knn_grid_kernel<1>, grid, block, 0, st, a);
    else if (k <= 4) hipLaunchKernelGGL(knn_grid_kernel<4>, grid, block, 0, st, a);
    else if (k <= 8) hipLaunchKernelGGL(knn_grid_kernel<8>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(knn_grid_kernel<16>, grid, block, 0, st, a);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_knn_blend(const void* values, int value_bytes, int64_t n, int64_t n_cols, const int32_t* idx, const float* dist2,
                             const int32_t* count, int64_t m, int k, int inverse, float eps, float fill, void* out, uint8_t* found,
                             int32_t* err, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t lim = int64_t(1) << 31;
    OSN_REQUIRE(value_bytes == 2 || value_bytes == 4, OSN_E_ARG, "osn_knn_blend: values are fp16 (2) or fp32 (4), got %d bytes", value_bytes);
    OSN_REQUIRE(n >= 0 && n < lim && m >= 0 && m < lim / KNN_MAX_K && n_cols >= 1 && n_cols < lim, OSN_E_ARG,
                "osn_knn_blend: sizes out of range (n=%lld m=%lld n_cols=%lld)", (long long)n, (long long)m, (long long)n_cols);
    OSN_REQUIRE(k >= 1 && k <= KNN_MAX_K, OSN_E_ARG, "osn_knn_blend: k=%d outside 1 .. %d", k, KNN_MAX_K);
    OSN_REQUIRE(inverse == 0 || (eps > 0.f && eps - eps == 0.f), OSN_E_ARG, "osn_knn_blend: inverse weights need a finite eps > 0");
    OSN_REQUIRE(err, OSN_E_ARG, "osn_knn_blend: null err");
    if (m == 0) return OSN_OK;
    OSN_REQUIRE(idx && dist2 && count && out && found && (n == 0 || values), OSN_E_ARG, "osn_knn_blend: null pointer");
    const bool wide = aligned16(values) && aligned16(out) && n_cols % (16 / value_bytes) == 0;     // 16-byte units, else single values
    if (value_bytes == 2) {
        if (wide) blend_launch<__half, 8>(st, values, n, n_cols, idx, dist2, count, m, k, inverse, eps, fill, out, found, err);
        else blend_launch<__half, 1>(st, values, n, n_cols, idx, dist2, count, m, k, inverse, eps, fill, out, found, err);
    } else {
        if (wide) blend_launch<float, 4>(st, values, n, n_cols, idx, dist2, count, m, k, inverse, eps, fill, out, found, err);
        else blend_launch<float, 1>(st, values, n, n_cols, idx, dist2, count, m, k, inverse, eps, fill, out, found, err);
    }
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_knn_vote(const int64_t* labels, int64_t n, const int32_t* idx, const int32_t* count, int64_t m, int k, int64_t fill,
                            int64_t* out, int32_t* err, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t lim = int64_t(1) << 31;
    OSN_REQUIRE(n >= 0 && n < lim && m >= 0 && m < lim / KNN_MAX_K, OSN_E_ARG, "osn_knn_vote: sizes out of range (n=%lld m=%lld)",
                (long long)n, (long long)m);
    OSN_REQUIRE(k >= 1 && k <= KNN_MAX_K, OSN_E_ARG, "osn_knn_vote: k=%d outside 1 .. %d", k, KNN_MAX_K);
    OSN_REQUIRE(err, OSN_E_ARG, "osn_knn_vote: null err");
    if (m == 0) return OSN_OK;
    OSN_REQUIRE(idx && count && out && (n == 0 || labels), OSN_E_ARG, "osn_knn_vote: null pointer");
    hipLaunchKernelGGL(knn_vote_kernel, dim3(unsigned(cdiv(m, KNN_T))), dim3(KNN_T), 0, st, labels, n, idx, count, m, k, fill, out, err);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}
