// Scene views on gfx950: a point-splat rasteriser with an exact z-buffer, and the pass that shades it (the picture of the
// reference's demo -- the regions matching a typed phrase, highlighted -- and the depth image PointCloudToImageMapper's
// occlusion test wants when a scan brings none, as scripts/feature_fusion/nuscenes_openseg.py does not).
//
//   osn_render_splat   zbuf[v, y, x] = min over the points covering the pixel of (bits of float32(depth) << 32 | point index)
//   osn_render_shade   zbuf -> point_id, depth, and rgb from colours / labels through a palette / a heat column through a LUT
//
// Splat.  The key orders by depth first (positive floats order as their bit patterns), by point index among equal float32
// depths, and the z-buffer is the 64-bit unsigned minimum of the keys of every point whose footprint covers the pixel: a
// pure function of the inputs, whatever order the atomics land in.  The centre pixel comes from project.h, the body
// osn_fusion_project runs, so it is bit for bit the pixel compute_mapping gives the point.
//
// Work layout.  A workgroup takes 256 points; a lane projects one point and writes its header (centre, pixel radius, the
// rows of its footprint that lie inside the image) to LDS.  The footprints are then swept as (point, row) pairs dealt to
// the lanes round robin through a prefix sum of the row counts: a lane walks ONE row of one footprint (at most 2 r + 1 <=
// 33 pixels), so a near point with a disc of 800 pixels is spread over 33 lanes instead of holding 63 idle ones, and with
// radius 0 every lane has exactly one pixel.  The atomics return nothing, so a lane issues its row without waiting.
// A load of the pixel in front of each atomic, skipping it when the stored key is already smaller (safe: the word only ever
// decreases), was measured and left out: on the 150 k-point room, 8 views of 640 x 480, it made the pass SLOWER (86 -> 102
// us at radius 0, 335 -> 423 us at 2 cm) -- the load's latency sits in front of every atomic of the row.
//
// Shade.  One lane per pixel; everything is an integer or a selected input value.  The heat index is
// t = (float(h) - lo) / (hi - lo) with correctly rounded fp32 operations, then rint(t * 255) clamped to 255.
#include "project.h"
#include <hip/hip_fp16.h>

namespace osn {

using u64 = unsigned long long;
constexpr int RS_T = 256;
constexpr int RENDER_MAX_PX = 16;
constexpr int SHADE_NONE = 0, SHADE_COLORS = 1, SHADE_LABELS = 2, SHADE_HEAT = 3;

struct SplatArgs {
    Pinhole cam;
    double radius_fx;      // radius * fx, one IEEE multiply (0 when radius == 0)
    double near;
    int H, W, max_px;
};

__global__ __launch_bounds__(RS_T) void render_splat_kernel(const double* __restrict__ coords, int64_t n, SplatArgs a, u64* z) {
    __shared__ int s_u[RS_T], s_v[RS_T], s_r[RS_T], s_y0[RS_T], s_end[RS_T], s_wave[RS_T / 64];
    __shared__ uint32_t s_z[RS_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = int64_t(blockIdx.x) * RS_T;
    const int64_t i = base + tid;
    int rows = 0;
    if (i < n) {
        const Projected q = project_point(coords, i, a.cam);
        const float zf = __double2float_rn(q.p2);
        const double lim = double(1 << 30);
        // NaN fails p2 >= near and both |.| < 2^30
        if (q.p2 >= a.near && !isinf(zf) && fabs(q.ur) < lim && fabs(q.vr) < lim) {
            int r = 0;
            if (a.radius_fx != 0.0) {
                const double rr = rint(__ddiv_rn(a.radius_fx, q.p2));
                r = rr >= double(a.max_px) ? a.max_px : (rr > 0.0 ? int(rr) : 0);      // (NaN -> 0)
            }
            const int u = int(q.ur), v = int(q.vr);
            const int y0 = max(v - r, 0), y1 = min(v + r, a.H - 1);
            // a footprint wholly left or right of the image draws nothing
            if (y1 >= y0 && u + r >= 0 && u - r <= a.W - 1) {
                rows = y1 - y0 + 1;
                s_u[tid] = u; s_v[tid] = v; s_r[tid] = r; s_y0[tid] = y0;
                s_z[tid] = __float_as_uint(zf);
            }
        }
    }
    int incl = rows;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int k = 0; k < RS_T / 64; ++k) {
        if (k < wave) off += s_wave[k];
        total += s_wave[k];
    }
    s_end[tid] = off + incl;
    __syncthreads();
    for (int it = tid; it < total; it += RS_T) {
        int lo = 0, hi = RS_T - 1;                           // the first point whose rows end after `it`
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_end[mid] > it) hi = mid; else lo = mid + 1;
        }
        const int j = lo;
        const int first = j ? s_end[j - 1] : 0;
        const int y = s_y0[j] + (it - first);
        const int dy = y - s_v[j], r = s_r[j], u = s_u[j];
        const int w = int(__fsqrt_rn(float(r * r - dy * dy)));          // exact: an integer <= 256
        const int x0 = max(u - w, 0), x1 = min(u + w, a.W - 1);
        const u64 key = (u64(s_z[j]) << 32) | u64(uint32_t(base + j));
        const int64_t row = int64_t(y) * a.W;
        for (int x = x0; x <= x1; ++x) atomicMin(z + row + x, key);
    }
}

struct ShadeArgs {
    int mode;
    const uint8_t* colors;       // colours [n, 3], or the base of the heat mode (nullable there)
    const void* values;          // labels int32 / int64, heat fp16 / fp32
    int value_bytes;
    int64_t offset, stride;      // element offset and stride of the values
    const uint8_t* table;        // palette [rows, 3] or LUT [256, 3]
    int table_rows;
    float lo, hi;
    uint32_t other, background;  // r | g << 8 | b << 16
};

__device__ inline uint32_t rgb_at(const uint8_t* __restrict__ t, int64_t row) {
    return uint32_t(t[3 * row]) | uint32_t(t[3 * row + 1]) << 8 | uint32_t(t[3 * row + 2]) << 16;
}

__global__ __launch_bounds__(RS_T) void render_shade_kernel(const u64* __restrict__ z, int64_t P, int64_t n, int32_t* __restrict__ point_id,
                                                            float* __restrict__ depth, uint8_t* __restrict__ rgb, ShadeArgs a) {
    const int64_t p = int64_t(blockIdx.x) * RS_T + threadIdx.x;
    if (p >= P) return;
    const u64 key = z[p];
    const bool bg = key == ~u64(0);
    const uint32_t id = uint32_t(key);
    point_id[p] = bg ? -1 : int32_t(id);
    depth[p] = bg ? 0.f : __uint_as_float(uint32_t(key >> 32));
    if (a.mode == SHADE_NONE) return;
    uint32_t c = a.background;
    if (!bg) {
        c = a.other;
        if (int64_t(id) < n) {                               // an id outside the arrays is never dereferenced
            const int64_t e = a.offset + int64_t(id) * a.stride;
            if (a.mode == SHADE_COLORS) {
                c = rgb_at(a.colors, id);
            } else if (a.mode == SHADE_LABELS) {
                const int64_t l = a.value_bytes == 8 ? static_cast<const int64_t*>(a.values)[e]
                                                     : int64_t(static_cast<const int32_t*>(a.values)[e]);
                if (l >= 0 && l < a.table_rows) c = rgb_at(a.table, l);
            } else {
                const float h = a.value_bytes == 2 ? __half2float(static_cast<const __half*>(a.values)[e])
                                                   : static_cast<const float*>(a.values)[e];
                if (h < a.lo) {
                    c = a.colors ? rgb_at(a.colors, id) : rgb_at(a.table, 0);
                } else if (h == h) {
                    const float t = __fdiv_rn(__fsub_rn(h, a.lo), __fsub_rn(a.hi, a.lo));
                    const float s = rintf(__fmul_rn(t, 255.f));
                    c = rgb_at(a.table, s >= 255.f ? 255 : int(s));
                }
            }
        }
    }
    rgb[3 * p + 0] = uint8_t(c); rgb[3 * p + 1] = uint8_t(c >> 8); rgb[3 * p + 2] = uint8_t(c >> 16);
}

}  // namespace osn

using namespace osn;

extern "C" int osn_render_splat(const double* coords3, int64_t n, const double* views20, int n_views, int H, int W, double radius,
                                int max_px, double near, uint64_t* zbuf, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(n >= 0 && n < (int64_t(1) << 32) - 1, OSN_E_ARG, "osn_render_splat: need 0 <= n < 2^32 - 1 (n=%lld)", (long long)n);
    OSN_REQUIRE(n_views >= 0 && H >= 1 && W >= 1 && int64_t(H) * W < (int64_t(1) << 31), OSN_E_ARG,
                "osn_render_splat: bad image sizes (views=%d H=%d W=%d)", n_views, H, W);
    OSN_REQUIRE(radius >= 0.0 && radius - radius == 0.0, OSN_E_ARG, "osn_render_splat: the radius must be finite and >= 0");
    OSN_REQUIRE(max_px >= 0 && max_px <= RENDER_MAX_PX, OSN_E_ARG, "osn_render_splat: max_px=%d outside 0 .. %d", max_px, RENDER_MAX_PX);
    OSN_REQUIRE(near > 0.0 && near - near == 0.0, OSN_E_ARG, "osn_render_splat: near must be finite and > 0");
    if (n_views == 0) return OSN_OK;
    OSN_REQUIRE(zbuf && views20, OSN_E_ARG, "osn_render_splat: null pointer");
    const int64_t plane = int64_t(H) * W;
    OSN_HIP(hipMemsetAsync(zbuf, 0xFF, size_t(n_views) * size_t(plane) * sizeof(uint64_t), st));      // all ones: background
    if (n == 0) return OSN_OK;
    OSN_REQUIRE(coords3, OSN_E_ARG, "osn_render_splat: null pointer");
    for (int v = 0; v < n_views; ++v) {
        const double* view = views20 + 20 * size_t(v);
        SplatArgs a;
        a.cam = make_pinhole(view, view + 16);
        a.radius_fx = radius == 0.0 ? 0.0 : radius * a.cam.fx;
        a.near = near;
        a.H = H; a.W = W; a.max_px = max_px;
        hipLaunchKernelGGL(render_splat_kernel, dim3(unsigned(cdiv(n, RS_T))), dim3(RS_T), 0, st, coords3, n, a,
                           reinterpret_cast<u64*>(zbuf) + v * plane);
    }
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_render_shade(const uint64_t* zbuf, int64_t n_pixels, int64_t n, int32_t* point_id, float* depth, uint8_t* rgb,
                                int mode, const uint8_t* colors, const void* values, int value_bytes, int64_t value_offset,
                                int64_t value_stride, const uint8_t* table, int table_rows, float lo, float hi, uint32_t other_rgb,
                                uint32_t background_rgb, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(n_pixels >= 0 && n >= 0 && n < (int64_t(1) << 31), OSN_E_ARG, "osn_render_shade: need n_pixels >= 0 and 0 <= n < 2^31");
    OSN_REQUIRE(mode >= SHADE_NONE && mode <= SHADE_HEAT, OSN_E_ARG, "osn_render_shade: mode=%d (0 none, 1 colours, 2 labels, 3 heat)", mode);
    if (n_pixels == 0) return OSN_OK;
    OSN_REQUIRE(zbuf && point_id && depth, OSN_E_ARG, "osn_render_shade: null pointer");
    OSN_REQUIRE(mode == SHADE_NONE || rgb, OSN_E_ARG, "osn_render_shade: null rgb");
    if (n > 0) {
        if (mode == SHADE_COLORS) OSN_REQUIRE(colors, OSN_E_ARG, "osn_render_shade: null colours");
        if (mode == SHADE_LABELS)
            OSN_REQUIRE(values && (value_bytes == 4 || value_bytes == 8) && table_rows >= 0 && (table || table_rows == 0), OSN_E_ARG,
                        "osn_render_shade: labels are int32 or int64 with a palette");
        if (mode == SHADE_HEAT) {
            OSN_REQUIRE(values && (value_bytes == 2 || value_bytes == 4) && table && table_rows == 256, OSN_E_ARG,
                        "osn_render_shade: heat values are fp16 or fp32 with a LUT of 256 rows");
            OSN_REQUIRE(hi > lo && hi - lo < __builtin_inff(), OSN_E_ARG, "osn_render_shade: need finite lo < hi");
        }
        if (mode >= SHADE_LABELS)
            OSN_REQUIRE(value_offset >= 0 && value_stride >= 1, OSN_E_ARG, "osn_render_shade: need offset >= 0 and stride >= 1");
    }
    ShadeArgs a;
    a.mode = mode; a.colors = colors; a.values = values; a.value_bytes = value_bytes; a.offset = value_offset; a.stride = value_stride;
    a.table = table; a.table_rows = table_rows; a.lo = lo; a.hi = hi; a.other = other_rgb; a.background = background_rgb;
    hipLaunchKernelGGL(render_shade_kernel, dim3(unsigned(cdiv(n_pixels, RS_T))), dim3(RS_T), 0, st,
                       reinterpret_cast<const u64*>(zbuf), n_pixels, n, point_id, depth, rgb, a);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}
