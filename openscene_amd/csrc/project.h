// The pinhole projection of one point, shared by the fusion mapping (fusion.hip) and the splat rasteriser (render.hip):
// one body, so a point's centre pixel in a rendered view is, bit for bit, the pixel compute_mapping gives it.
//
// fp64 exactly as numpy computes it (scripts/feature_fusion/fusion_util.py:103-116):
//   p = world_to_camera @ [x y z 1]^T     an FMA chain in dgemm's order (m0*x, then +m1*y, +m2*z, +m3*1 fused)
//   u = (p0 * fx) / p2 + cx               separate IEEE multiply, divide, add (numpy does not contract)
//   round half to even (np.round)
#pragma once
#include "common.h"

namespace osn {

struct Pinhole {
    double m[12];          // rows 0..2 of world_to_camera (row-major 3 x 4)
    double fx, fy, cx, cy;
};

struct Projected {
    double p2;             // camera-space depth
    double ur, vr;         // rounded pixel column / row (NaN / inf when the division gave one)
};

static inline Pinhole make_pinhole(const double* world_to_camera16, const double* intrinsic4) {
    Pinhole a;
    for (int i = 0; i < 12; ++i) a.m[i] = world_to_camera16[i];
    a.fx = intrinsic4[0]; a.fy = intrinsic4[1]; a.cx = intrinsic4[2]; a.cy = intrinsic4[3];
    return a;
}

__device__ inline Projected project_point(const double* __restrict__ coords, int64_t i, const Pinhole& a) {
    const double x = coords[3 * i + 0], y = coords[3 * i + 1], z = coords[3 * i + 2];
    double p[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double s = __dmul_rn(a.m[4 * r + 0], x);
        s = fma(a.m[4 * r + 1], y, s);
        s = fma(a.m[4 * r + 2], z, s);
        p[r] = fma(a.m[4 * r + 3], 1.0, s);
    }
    const double u = __dadd_rn(__ddiv_rn(__dmul_rn(p[0], a.fx), p[2]), a.cx);
    const double v = __dadd_rn(__ddiv_rn(__dmul_rn(p[1], a.fy), p[2]), a.cy);
    return Projected{p[2], rint(u), rint(v)};               // round half to even
}

}  // namespace osn
