// Elastic distortion of a point cloud on gfx950: dataset/augmentation.py:159-201 (ElasticDistortion.elastic_distortion),
// the pre-voxeliser transform of Point3DLoader (dataset/point_loader.py:156), bit-identical to numpy 2.2 / scipy 1.15
// given the same noise draw (the draw itself stays on the host, in numpy's order).
//
//   osn_bbox            coords.min(0), coords.max(0) of a float64 [n,3] cloud.  Min and max are exact in any order.
//   osn_elastic_blur    the six scipy.ndimage.convolve calls (3-tap box along x, y, z, twice) on the float32 noise grid,
//                       mode='constant', cval=0.  ndimage casts the float32 weight 1/3 to double, accumulates
//                       res = 0; res += w * v  over the taps at offsets -1, 0, +1 (an outside tap adds w * 0), then
//                       stores (float)res -- reproduced per pass, ping-ponging through the workspace.
//   osn_elastic_apply   RegularGridInterpolator(ax, noise, bounds_error=0, fill_value=0)(coords) * magnitude + coords,
//                       scipy's linear path for ndim 3 (_rgi.py _evaluate_linear, _rgi_cython find_indices):
//                         interval i with ax[i] <= x < ax[i+1], x == ax[-1] -> n-2;  y = (x - ax[i]) / (ax[i+1] - ax[i])
//                         corners in itertools.product order, weight = ((1 * w0) * w1) * w2, value = 0 + term + ...
//                         term = (double)noise_f32 * weight;  x < ax[0] or x > ax[-1] on any axis -> value 0
//                       and, in the same pass, the bounding box of the result (it sizes the next field's grid).
// hipcc contracts a*b+c to an FMA by default; numpy does not.  HIP's __dmul_rn / __dadd_rn are plain `*` / `+` defined
// in a header that is compiled with contraction on, so after inlining they fuse too.  Contraction is therefore switched off
// for this file and every float64 operation goes through the d_* helpers below (checked: no v_fma_f64 outside the
// division sequences in the ISA).
#include "common.h"

#pragma clang fp contract(off)

namespace osn {

__device__ inline double d_add(double a, double b) { return a + b; }
__device__ inline double d_sub(double a, double b) { return a - b; }
__device__ inline double d_mul(double a, double b) { return a * b; }
__device__ inline double d_div(double a, double b) { return a / b; }

constexpr int EL_BLOCK = 256;
constexpr int EL_MAX_BLOCKS = 2048;      // partial boxes per reduction: 2048 * 48 B of workspace

// ---- block-wide min / max of three axes; thread 0 writes lo[3], hi[3] to part[6] -------------------------------------
__device__ inline void block_box(double lo[3], double hi[3], double* __restrict__ part) {
    __shared__ double s[EL_BLOCK / 64][6];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double a = __shfl_xor(lo[d], off), b = __shfl_xor(hi[d], off);
            lo[d] = a < lo[d] ? a : lo[d];
            hi[d] = b > hi[d] ? b : hi[d];
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { s[wave][d] = lo[d]; s[wave][3 + d] = hi[d]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < EL_BLOCK / 64; ++w) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                lo[d] = s[w][d] < lo[d] ? s[w][d] : lo[d];
                hi[d] = s[w][3 + d] > hi[d] ? s[w][3 + d] : hi[d];
            }
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) { part[d] = lo[d]; part[3 + d] = hi[d]; }
    }
}

__global__ __launch_bounds__(EL_BLOCK) void bbox_partial_kernel(const double* __restrict__ xyz, int64_t n,
                                                                double* __restrict__ part) {
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (int64_t i = int64_t(blockIdx.x) * EL_BLOCK + threadIdx.x; i < n; i += int64_t(gridDim.x) * EL_BLOCK) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double v = xyz[3 * i + d];
            lo[d] = v < lo[d] ? v : lo[d];
            hi[d] = v > hi[d] ? v : hi[d];
        }
    }
    block_box(lo, hi, part + 6 * int64_t(blockIdx.x));
}

// one workgroup: the partial boxes of `nb` blocks -> bbox6 = (min x, min y, min z, max x, max y, max z)
__global__ __launch_bounds__(EL_BLOCK) void bbox_final_kernel(const double* __restrict__ part, int nb,
                                                              double* __restrict__ bbox6) {
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (int b = threadIdx.x; b < nb; b += EL_BLOCK) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double a = part[6 * b + d], c = part[6 * b + 3 + d];
            lo[d] = a < lo[d] ? a : lo[d];
            hi[d] = c > hi[d] ? c : hi[d];
        }
    }
    block_box(lo, hi, bbox6);
}

// one 3-tap pass along an axis of the [nx, ny, nz, 3] grid: `stride` elements between neighbours, `len` nodes on the axis
__global__ __launch_bounds__(EL_BLOCK) void blur_pass_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                             int64_t total, int64_t stride, int len) {
    const int64_t e = int64_t(blockIdx.x) * EL_BLOCK + threadIdx.x;
    if (e >= total) return;
    const double w = double(1.0f / 3.0f);                   // np.ones(...).astype('float32') / 3, cast to double by ndimage
    const int64_t pos = (e / stride) % len;
    const float vm = pos > 0 ? in[e - stride] : 0.0f;
    const float v0 = in[e];
    const float vp = pos < len - 1 ? in[e + stride] : 0.0f;
    double r = 0.0;
    r = d_add(r, d_mul(w, double(vm)));
    r = d_add(r, d_mul(w, double(v0)));
    r = d_add(r, d_mul(w, double(vp)));
    out[e] = __double2float_rn(r);
}

// interval of x on an ascending axis of n >= 2 nodes: ax[i] <= x < ax[i+1], clamped to [0, n-2] (scipy's
// find_interval_ascending; x == ax[n-1] and x beyond either end land on the clamps).  The guess from the uniform spacing
// is only a starting point: the two walks compare against the stored nodes, so the result does not depend on it.
__device__ inline int find_interval(const double* __restrict__ ax, int n, double x) {
    const double a0 = ax[0], step = (ax[n - 1] - a0) / double(n - 1);
    double gs = (x - a0) / step;
    gs = gs > 0.0 ? gs : 0.0;                               // also maps NaN to 0
    gs = gs < double(n - 2) ? gs : double(n - 2);
    int i = int(gs);
    while (i > 0 && x < ax[i]) --i;
    while (i < n - 2 && x >= ax[i + 1]) ++i;
    return i;
}

struct ApplyArgs {
    int nx, ny, nz;
    double magnitude;
};

__global__ __launch_bounds__(EL_BLOCK) void elastic_apply_kernel(const double* __restrict__ xyz, int64_t n,
                                                                 const float* __restrict__ noise,
                                                                 const double* __restrict__ axes, ApplyArgs a,
                                                                 double* __restrict__ out, double* __restrict__ part) {
    const int dims[3] = {a.nx, a.ny, a.nz};
    const double* axp[3] = {axes, axes + a.nx, axes + a.nx + a.ny};
    const int64_t sy = int64_t(a.nz) * 3, sx = int64_t(a.ny) * sy;
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (int64_t p = int64_t(blockIdx.x) * EL_BLOCK + threadIdx.x; p < n; p += int64_t(gridDim.x) * EL_BLOCK) {
        double x[3], y[3];
        int idx[3];
        bool oob = false;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            x[d] = xyz[3 * p + d];
            const double* g = axp[d];
            const int i = find_interval(g, dims[d], x[d]);
            const double g0 = g[i], g1 = g[i + 1];
            idx[d] = i;
            y[d] = d_div(d_sub(x[d], g0), d_sub(g1, g0));
            oob = oob || x[d] < g[0] || x[d] > g[dims[d] - 1];
        }
        double v[3] = {0.0, 0.0, 0.0};
        if (!oob) {
            const double w1[3] = {d_sub(1.0, y[0]), d_sub(1.0, y[1]), d_sub(1.0, y[2])};
            const float* base = noise + idx[0] * sx + idx[1] * sy + int64_t(idx[2]) * 3;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int b0 = (c >> 2) & 1, b1 = (c >> 1) & 1, b2 = c & 1;
                double w = d_mul(1.0, b0 ? y[0] : w1[0]);
                w = d_mul(w, b1 ? y[1] : w1[1]);
                w = d_mul(w, b2 ? y[2] : w1[2]);
                const float* q = base + b0 * sx + b1 * sy + b2 * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) v[k] = d_add(v[k], d_mul(double(q[k]), w));
            }
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double o = d_add(x[d], d_mul(v[d], a.magnitude));
            out[3 * p + d] = o;
            lo[d] = o < lo[d] ? o : lo[d];
            hi[d] = o > hi[d] ? o : hi[d];
        }
    }
    block_box(lo, hi, part + 6 * int64_t(blockIdx.x));
}

static int reduction_blocks(int64_t n) {
    int64_t b = cdiv(n, EL_BLOCK);
    return int(b < EL_MAX_BLOCKS ? b : EL_MAX_BLOCKS);
}

}  // namespace osn

using namespace osn;

extern "C" size_t osn_bbox_ws_bytes(int64_t n) {
    return size_t(reduction_blocks(n > 0 ? n : 1)) * 6 * sizeof(double);
}

extern "C" int osn_bbox(const double* xyz, int64_t n, double* bbox6, void* ws, size_t ws_bytes, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(n >= 1, OSN_E_ARG, "osn_bbox: the cloud is empty (numpy's min of an empty array raises)");
    OSN_REQUIRE(xyz && bbox6 && ws, OSN_E_ARG, "osn_bbox: null pointer");
    OSN_REQUIRE(ws_bytes >= osn_bbox_ws_bytes(n), OSN_E_WS, "osn_bbox: workspace too small");
    const int nb = reduction_blocks(n);
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(bbox_partial_kernel, dim3(nb), dim3(EL_BLOCK), 0, st, xyz, n, part);
    OSN_LAUNCH_CHECK();
    hipLaunchKernelGGL(bbox_final_kernel, dim3(1), dim3(EL_BLOCK), 0, st, part, nb, bbox6);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" size_t osn_elastic_blur_ws_bytes(int nx, int ny, int nz) {
    if (nx < 1 || ny < 1 || nz < 1) return 0;
    return size_t(nx) * size_t(ny) * size_t(nz) * 3 * sizeof(float);
}

extern "C" int osn_elastic_blur(float* noise, int nx, int ny, int nz, void* ws, size_t ws_bytes, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, OSN_E_ARG, "osn_elastic_blur: bad grid %d x %d x %d", nx, ny, nz);
    const int64_t total = int64_t(nx) * ny * nz * 3;
    OSN_REQUIRE(total < (int64_t(1) << 40), OSN_E_ARG, "osn_elastic_blur: grid too large");
    OSN_REQUIRE(noise && ws, OSN_E_ARG, "osn_elastic_blur: null pointer");
    OSN_REQUIRE(ws_bytes >= osn_elastic_blur_ws_bytes(nx, ny, nz), OSN_E_WS, "osn_elastic_blur: workspace too small");
    float* tmp = static_cast<float*>(ws);
    const int len[3] = {nx, ny, nz};
    const int64_t stride[3] = {int64_t(ny) * nz * 3, int64_t(nz) * 3, 3};
    const unsigned blocks = unsigned(cdiv(total, EL_BLOCK));
    for (int rep = 0; rep < 2; ++rep) {
        for (int ax = 0; ax < 3; ++ax) {                    // passes 1, 3, 5: noise -> tmp; 2, 4, 6: tmp -> noise
            const int k = rep * 3 + ax;
            const float* src = (k & 1) ? tmp : noise;
            float* dst = (k & 1) ? noise : tmp;
            hipLaunchKernelGGL(blur_pass_kernel, dim3(blocks), dim3(EL_BLOCK), 0, st, src, dst, total, stride[ax], len[ax]);
            OSN_LAUNCH_CHECK();
        }
    }
    return OSN_OK;
}

extern "C" size_t osn_elastic_apply_ws_bytes(int64_t n) { return osn_bbox_ws_bytes(n); }

extern "C" int osn_elastic_apply(const double* xyz, int64_t n, const float* noise, int nx, int ny, int nz,
                                 const double* axes, double magnitude, double* out, double* bbox6, void* ws,
                                 size_t ws_bytes, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(n >= 1, OSN_E_ARG, "osn_elastic_apply: the cloud is empty");
    OSN_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, OSN_E_ARG, "osn_elastic_apply: every axis needs >= 2 nodes (%d, %d, %d)",
                nx, ny, nz);
    OSN_REQUIRE(int64_t(nx) * ny * nz * 3 < (int64_t(1) << 40), OSN_E_ARG, "osn_elastic_apply: grid too large");
    OSN_REQUIRE(xyz && noise && axes && out && bbox6 && ws, OSN_E_ARG, "osn_elastic_apply: null pointer");
    OSN_REQUIRE(out != xyz, OSN_E_ARG, "osn_elastic_apply: out must not alias xyz");
    OSN_REQUIRE(ws_bytes >= osn_elastic_apply_ws_bytes(n), OSN_E_WS, "osn_elastic_apply: workspace too small");
    const int nb = reduction_blocks(n);
    double* part = static_cast<double*>(ws);
    ApplyArgs a;
    a.nx = nx; a.ny = ny; a.nz = nz;
    a.magnitude = magnitude;
    hipLaunchKernelGGL(elastic_apply_kernel, dim3(nb), dim3(EL_BLOCK), 0, st, xyz, n, noise, axes, a, out, part);
    OSN_LAUNCH_CHECK();
    hipLaunchKernelGGL(bbox_final_kernel, dim3(1), dim3(EL_BLOCK), 0, st, part, nb, bbox6);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}
