// Points in and out of the voxel grid on gfx950 ([ME] TensorField / .sparse(), SparseTensor.slice(), SparseTensor.interpolate(),
// MinkowskiInterpolation, features_at_coordinates; run/evaluate.py:283-292 reads predictions[inds_reverse] instead).
//
//   osn_field_map       per position the eight corners of its cell in a stride-s coordinate table and their trilinear weights:
//                       q = p / float(s), f = floorf(q), base = int(f) s, t = q - f, a[0] = 1 - t, a[1] = t per axis,
//                       corner k = dx + 2 dy + 4 dz at base + s (dx, dy, dz), w[k] = (ax[dx] ay[dy]) az[dz].  One thread per
//                       position: the range test, eight probes, eight weights.  A row that is not finite, whose batch is
//                       outside [0, 65535) or whose base or base + s leaves (-32767, 32767) has no corner and weight +0 and is
//                       counted in `bad` (an integer atomic): the range test comes BEFORE pack_key, which wraps at 16 bits.
//   osn_interp_fwd      y[m] = sum over the present k, ascending, from +0, of w[k, m] x[nbr[k, m]]; the layout of pool_fwd_kernel
//                       (csrc/pooling.hip): one thread per row and four columns, the corners' loads issued before the adds.
//   osn_interp_bwd      gx[v] = sum over the pairs e = k m_rows + m with nbr[k, m] = v, ascending e, from +0, of w[e] gy[m]:
//                       one thread per voxel row and four columns walks the row's list of a plan sorted by (voxel row, e).
//   osn_segment_reduce  y[u] = the rows order[offsets[u] .. offsets[u + 1]) of x added one by one from +0 (avg: one division by
//                       float(length)): the sum / average quantisation of a field and the backward pass of a slice.  One thread
//                       per segment and four columns: about 1.2 points fall into a voxel, a chunked reduction would give every
//                       segment a workgroup.  A voxel with hundreds of points runs serially in its threads: correct, and slow.
//
// No floating-point atomics and no LDS: every result is a pure function of its arguments.  wave64, 16-byte accesses when
// c % 4 == 0 and the matrices are 16-byte aligned, one element per thread otherwise.
#include "common.h"

// Every float32 operation of this file rounds on its own (the weights' two products, each term's product and its add).  The
// operators are written plainly under this pragma: the __fmul_rn / __fadd_rn intrinsics are operators inside a header, compiled
// under the default, which contracts them into FMA.
#pragma clang fp contract(off)

namespace osn {

enum { SEG_SUM = OSN_SEGMENT_SUM, SEG_AVG = OSN_SEGMENT_AVG };
constexpr int FD_T = 256;
constexpr int64_t FD_MAX_ROWS = (int64_t(1) << 31) - 1;
constexpr int64_t FD_MAX_THREADS = (int64_t(1) << 31) * FD_T - FD_T;
constexpr int64_t FD_MAX_POINTS = ((int64_t(1) << 31) - 1) / 8;         // 8 m is an int32 pair index

template <int V, typename T>
__device__ inline void fd_ld(const T* __restrict__ p, T (&v)[V]) {
    static_assert(sizeof(T) == 4, "32-bit elements");
    if constexpr (V == 4) {
        const uint4 t = *reinterpret_cast<const uint4*>(p);
        v[0] = __builtin_bit_cast(T, t.x); v[1] = __builtin_bit_cast(T, t.y);
        v[2] = __builtin_bit_cast(T, t.z); v[3] = __builtin_bit_cast(T, t.w);
    } else {
        v[0] = *p;
    }
}
template <int V, typename T>
__device__ inline void fd_st(T* __restrict__ p, const T (&v)[V]) {
    if constexpr (V == 4) {
        *reinterpret_cast<uint4*>(p) = make_uint4(__builtin_bit_cast(uint32_t, v[0]), __builtin_bit_cast(uint32_t, v[1]),
                                                  __builtin_bit_cast(uint32_t, v[2]), __builtin_bit_cast(uint32_t, v[3]));
    } else {
        *p = v[0];
    }
}
// an index that names a row of [0, rows): -1 and anything else outside count as absent
__device__ inline bool fd_row_ok(int64_t i, int64_t rows) { return uint64_t(i) < uint64_t(rows); }
__device__ inline bool fd_finite(float v) { return v - v == 0.f; }

// a list range of a CSR, held inside [0, n] whatever the offsets say
__device__ inline void fd_range(const int64_t* __restrict__ offsets, int64_t u, int64_t n, int64_t& lo, int64_t& hi) {
    lo = offsets[u];
    hi = offsets[u + 1];
    lo = lo < 0 ? 0 : (lo > n ? n : lo);
    hi = hi < lo ? lo : (hi > n ? n : hi);
}

// one axis: the cell's base coordinate and the two weights; false if base or base + s leaves (-32767, 32767)
__device__ inline bool fd_axis(float p, float fs, int s, int& base, float (&a)[2]) {
    const float q = __fdiv_rn(p, fs);
    const float f = floorf(q);
    if (!(f > -32768.f && f < 32768.f)) return false;                  // (also a NaN: the conversion below is defined)
    const int64_t b = int64_t(int(f)) * s;
    const int64_t lim = COORD_BIAS - 1;
    if (!(b > -lim && b + s < lim)) return false;
    base = int(b);
    const float t = q - f;
    a[0] = 1.f - t;
    a[1] = t;
    return true;
}

__global__ __launch_bounds__(FD_T) void field_map_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals,
                                                         uint32_t mask, const float* __restrict__ coords4f, int64_t m, int stride,
                                                         int32_t* __restrict__ nbr, float* __restrict__ w, int32_t* __restrict__ bad) {
    const int64_t i = int64_t(blockIdx.x) * FD_T + threadIdx.x;
    if (i >= m) return;
    const float pb = coords4f[4 * i], px = coords4f[4 * i + 1], py = coords4f[4 * i + 2], pz = coords4f[4 * i + 3];
    const float fs = float(stride);
    int bx = 0, by = 0, bz = 0;
    float ax[2], ay[2], az[2];
    bool ok = fd_finite(pb) && fd_finite(px) && fd_finite(py) && fd_finite(pz) && pb >= 0.f && pb < 65535.f;
    ok = ok && fd_axis(px, fs, stride, bx, ax) && fd_axis(py, fs, stride, by, ay) && fd_axis(pz, fs, stride, bz, az);
    if (!ok) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            nbr[int64_t(k) * m + i] = -1;
            w[int64_t(k) * m + i] = 0.f;
        }
        atomicAdd(bad, 1);
        return;
    }
    const int b = int(pb);
    int r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)                                        // eight independent probes, then the stores
        r[k] = table_find(keys, vals, mask, pack_key(b, bx + (k & 1) * stride, by + ((k >> 1) & 1) * stride, bz + (k >> 2) * stride));
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float wxy = ax[k & 1] * ay[(k >> 1) & 1];
        nbr[int64_t(k) * m + i] = r[k];
        w[int64_t(k) * m + i] = wxy * az[k >> 2];
    }
}

// one thread per (position, V columns)
template <int V>
__global__ __launch_bounds__(FD_T) void interp_fwd_kernel(const float* __restrict__ x, int64_t n_in, const int32_t* __restrict__ nbr,
                                                          const float* __restrict__ w, int64_t m, int c, int cg, float* __restrict__ y) {
    const int64_t e = int64_t(blockIdx.x) * FD_T + threadIdx.x;
    if (e >= m * cg) return;
    const int64_t o = e / cg;
    const int col = int(e - o * cg) * V;
    int idx[8];
    float wk[8], v[8][V], acc[V];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int i = nbr[int64_t(k) * m + o];
        idx[k] = fd_row_ok(i, n_in) ? i : -1;
        wk[k] = w[int64_t(k) * m + o];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {                       // every present corner's load, then the terms in order
        if (idx[k] >= 0) {
            fd_ld<V>(x + int64_t(idx[k]) * c + col, v[k]);
        } else {
#pragma unroll
            for (int u = 0; u < V; ++u) v[k][u] = 0.f;
        }
    }
#pragma unroll
    for (int u = 0; u < V; ++u) acc[u] = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (idx[k] < 0) continue;
#pragma unroll
        for (int u = 0; u < V; ++u) acc[u] += wk[k] * v[k][u];
    }
    fd_st<V>(y + o * c + col, acc);
}

// one thread per (voxel row, V columns): the row's pairs in list order, four in flight.  Every element of gx is written.
template <int V>
__global__ __launch_bounds__(FD_T) void interp_bwd_kernel(const float* __restrict__ gy, int64_t m, int c, int cg,
                                                          const int32_t* __restrict__ pair, int64_t n_pair,
                                                          const int64_t* __restrict__ offsets, const float* __restrict__ w, int64_t n_in,
                                                          float* __restrict__ gx) {
    const int64_t t = int64_t(blockIdx.x) * FD_T + threadIdx.x;
    if (t >= n_in * cg) return;
    const int64_t v = t / cg;
    const int col = int(t - v * cg) * V;
    int64_t lo, hi;
    fd_range(offsets, v, n_pair, lo, hi);
    float acc[V];
#pragma unroll
    for (int u = 0; u < V; ++u) acc[u] = 0.f;
    for (int64_t j0 = lo; j0 < hi; j0 += 4) {
        int64_t row[4];
        float wk[4], g[4][V];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t e = j0 + q < hi ? int64_t(pair[j0 + q]) : -1;
            const bool ok = fd_row_ok(e, 8 * m);
            row[q] = ok ? int64_t(uint32_t(e) % uint32_t(m)) : -1;      // (8 m < 2^31: a 32-bit remainder)
            wk[q] = ok ? w[e] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (row[q] >= 0) fd_ld<V>(gy + row[q] * c + col, g[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (row[q] < 0) continue;
#pragma unroll
            for (int u = 0; u < V; ++u) acc[u] += wk[q] * g[q][u];
        }
    }
    fd_st<V>(gx + v * c + col, acc);
}

// one thread per (segment, V columns): the segment's rows in list order, four in flight
template <int V, int MODE>
__global__ __launch_bounds__(FD_T) void segment_reduce_kernel(const float* __restrict__ x, int64_t n, int c, int cg,
                                                              const int32_t* __restrict__ order, const int64_t* __restrict__ offsets,
                                                              int64_t n_seg, float* __restrict__ y) {
    const int64_t t = int64_t(blockIdx.x) * FD_T + threadIdx.x;
    if (t >= n_seg * cg) return;
    const int64_t s = t / cg;
    const int col = int(t - s * cg) * V;
    int64_t lo, hi;
    fd_range(offsets, s, n, lo, hi);
    float acc[V];
#pragma unroll
    for (int u = 0; u < V; ++u) acc[u] = 0.f;
    for (int64_t j0 = lo; j0 < hi; j0 += 4) {
        int row[4];
        float v[4][V];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = j0 + q < hi ? order[j0 + q] : -1;
            row[q] = fd_row_ok(i, n) ? i : -1;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (row[q] >= 0) fd_ld<V>(x + int64_t(row[q]) * c + col, v[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (row[q] < 0) continue;
#pragma unroll
            for (int u = 0; u < V; ++u) acc[u] += v[q][u];
        }
    }
    if (MODE == SEG_AVG) {
        const float len = float(hi - lo);
#pragma unroll
        for (int u = 0; u < V; ++u) acc[u] = hi > lo ? __fdiv_rn(acc[u], len) : 0.f;
    }
    fd_st<V>(y + s * c + col, acc);
}

static bool fd_vec(int c, const void* a, const void* b) { return (c & 3) == 0 && aligned16(a) && aligned16(b); }

}  // namespace osn

using namespace osn;

extern "C" int osn_field_map(const uint64_t* table_keys, const int32_t* table_vals, int64_t cap, const float* coords4f, int64_t m,
                             int stride, int32_t* nbr, float* w, int32_t* bad, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(stride >= 1 && stride < COORD_BIAS, OSN_E_ARG, "osn_field_map: stride=%d (1 <= stride < 32768)", stride);
    OSN_REQUIRE(m >= 0 && m <= FD_MAX_POINTS, OSN_E_ARG, "osn_field_map: need 0 <= m and 8 m < 2^31 (m=%lld)", (long long)m);
    OSN_REQUIRE(cap >= 2 && (cap & (cap - 1)) == 0 && cap <= (int64_t(1) << 32), OSN_E_ARG,
                "osn_field_map: cap=%lld must be a power of two", (long long)cap);
    if (m == 0) return OSN_OK;
    OSN_REQUIRE(table_keys && table_vals && coords4f && nbr && w && bad, OSN_E_ARG, "osn_field_map: null pointer");
    hipLaunchKernelGGL(field_map_kernel, dim3(unsigned(cdiv(m, FD_T))), dim3(FD_T), 0, st, table_keys, table_vals, uint32_t(cap - 1),
                       coords4f, m, stride, nbr, w, bad);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_interp_fwd(const float* x, int64_t n_in, const int32_t* nbr, const float* w, int64_t m, int c, float* y,
                              osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(n_in >= 0 && n_in <= FD_MAX_ROWS && m >= 0 && m <= FD_MAX_POINTS && c >= 1 && m * int64_t(c) <= FD_MAX_THREADS, OSN_E_ARG,
                "osn_interp_fwd: need 0 <= n_in < 2^31, 0 <= 8 m < 2^31 and c >= 1 (n_in=%lld m=%lld c=%d)", (long long)n_in,
                (long long)m, c);
    if (m == 0) return OSN_OK;
    OSN_REQUIRE(nbr && w && y && (x || n_in == 0), OSN_E_ARG, "osn_interp_fwd: null pointer");
    const bool vec = fd_vec(c, x, y);
    const int cg = vec ? c / 4 : c;
    const dim3 grid(unsigned(cdiv(m * cg, FD_T)));
    if (vec) hipLaunchKernelGGL(interp_fwd_kernel<4>, grid, dim3(FD_T), 0, st, x, n_in, nbr, w, m, c, cg, y);
    else hipLaunchKernelGGL(interp_fwd_kernel<1>, grid, dim3(FD_T), 0, st, x, n_in, nbr, w, m, c, cg, y);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_interp_bwd(const float* gy, int64_t m, int c, const int32_t* pair, int64_t n_pair, const int64_t* offsets,
                              const float* w, int64_t n_in, float* gx, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(n_in >= 0 && n_in <= FD_MAX_ROWS && m >= 0 && m <= FD_MAX_POINTS && c >= 1 && n_in * int64_t(c) <= FD_MAX_THREADS &&
                    n_pair >= 0 && n_pair <= 8 * m,
                OSN_E_ARG, "osn_interp_bwd: need 0 <= n_in < 2^31, 0 <= 8 m < 2^31, 0 <= n_pair <= 8 m and c >= 1 (n_in=%lld m=%lld n_pair=%lld c=%d)",
                (long long)n_in, (long long)m, (long long)n_pair, c);
    if (n_in == 0) return OSN_OK;
    OSN_REQUIRE(offsets && gx && (n_pair == 0 || (gy && pair && w)), OSN_E_ARG, "osn_interp_bwd: null pointer");
    const bool vec = fd_vec(c, gy, gx);
    const int cg = vec ? c / 4 : c;
    const dim3 grid(unsigned(cdiv(n_in * cg, FD_T)));
    if (vec) hipLaunchKernelGGL(interp_bwd_kernel<4>, grid, dim3(FD_T), 0, st, gy, m, c, cg, pair, n_pair, offsets, w, n_in, gx);
    else hipLaunchKernelGGL(interp_bwd_kernel<1>, grid, dim3(FD_T), 0, st, gy, m, c, cg, pair, n_pair, offsets, w, n_in, gx);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_segment_reduce(const float* x, int64_t n, int c, const int32_t* order, const int64_t* offsets, int64_t n_seg, int mode,
                                  float* y, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(mode == SEG_SUM || mode == SEG_AVG, OSN_E_ARG, "osn_segment_reduce: mode %d (0 sum, 1 avg)", mode);
    OSN_REQUIRE(n >= 0 && n <= FD_MAX_ROWS && n_seg >= 0 && n_seg <= FD_MAX_ROWS && c >= 1 && n_seg * int64_t(c) <= FD_MAX_THREADS, OSN_E_ARG,
                "osn_segment_reduce: need 0 <= n, n_seg < 2^31 and c >= 1 (n=%lld n_seg=%lld c=%d)", (long long)n, (long long)n_seg, c);
    if (n_seg == 0) return OSN_OK;
    OSN_REQUIRE(offsets && y && (n == 0 || (x && order)), OSN_E_ARG, "osn_segment_reduce: null pointer");
    const bool vec = fd_vec(c, x, y);
    const int cg = vec ? c / 4 : c;
    const dim3 grid(unsigned(cdiv(n_seg * cg, FD_T)));
    if (vec && mode == SEG_AVG) hipLaunchKernelGGL((segment_reduce_kernel<4, SEG_AVG>), grid, dim3(FD_T), 0, st, x, n, c, cg, order, offsets, n_seg, y);
    else if (vec) hipLaunchKernelGGL((segment_reduce_kernel<4, SEG_SUM>), grid, dim3(FD_T), 0, st, x, n, c, cg, order, offsets, n_seg, y);
    else if (mode == SEG_AVG) hipLaunchKernelGGL((segment_reduce_kernel<1, SEG_AVG>), grid, dim3(FD_T), 0, st, x, n, c, cg, order, offsets, n_seg, y);
    else hipLaunchKernelGGL((segment_reduce_kernel<1, SEG_SUM>), grid, dim3(FD_T), 0, st, x, n, c, cg, order, offsets, n_seg, y);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}
