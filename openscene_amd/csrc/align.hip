// Two scans in one frame on gfx950: the rigid motion that takes matched points of one scan onto the other (RANSAC over
// triplets of correspondences), and the sums a least-squares polish of it needs (Kabsch on the host, ICP on the voxel index).
//
//   osn_rigid_from_triplets   per hypothesis the motion that takes one triangle of pairs onto the other, in float64
//   osn_rigid_score           per hypothesis the number of pairs it moves to within the threshold: H x P residuals
//   osn_rigid_best            the largest count and the lowest hypothesis that has it
//   osn_rigid_moments         under ONE transform: the inlier mask, the residuals, and over the inliers n, sum s, sum d, sum s d^T
//
// The contract (include/openscene_amd.h repeats it beside the entries).  A transform is 12 float32: R row-major, then t.
// The residual of a pair (s, d) is, in float32 with every operation rounded on its own,
//     x_i = ((R_i0 s_0) + (R_i1 s_1)) + (R_i2 s_2)      e_i = (x_i + t_i) - d_i      r2 = ((e_0 e_0) + (e_1 e_1)) + (e_2 e_2)
// and the pair is an inlier iff r2 <= tau2 (a NaN never is).  numpy float32 restates it bit for bit, so counts and masks are
// exact integers, the same on every call and on every schedule.  The triplet fit is separately rounded float64 in the order
// written in rigid_frame / rigid_from_triplets_kernel below.
//
// Every floating-point operation of this file rounds on its own: contraction into FMA is switched off for the file and the
// operators are written plainly (the __fmul_rn / __dmul_rn intrinsics are operators inside a header, compiled under the
// default, which contracts them).  The price is stated, not worked around: a residual is 9 multiplies, 9 additions and 3
// subtractions, 21 VALU operations and a compare where a fused form would need 15 and a compare.
//
// Score layout.  The grid is (pair tiles, hypothesis tiles).  A workgroup of four waves keeps RS_PT = 1024 pairs in registers,
// four per lane (24 VGPRs), and walks RS_HT = 64 hypotheses whose 12 values lie in LDS: three wave-uniform 16-byte reads
// (broadcasts) per hypothesis against 4 x 22 VALU instructions.  The compare goes to a lane mask, its population count is a
// scalar instruction; the wave's count of hypothesis hh is parked in lane hh's register, so the loop holds no atomic at all.
// After the loop a lane adds its register into the tile's LDS counter (one integer add per wave and hypothesis) and 64 lanes
// add the counters into `counts` (one integer atomicAdd per workgroup and hypothesis).  Integer atomics are exact and
// order-free.  A lane past P holds NaN pairs, which are inliers of nothing.
//
// Moments layout.  A chunk of OSN_RIGID_MOMENTS_CHUNK = 1024 pairs per workgroup: lane tid takes pairs tid, tid + 256, .. in order, the 64
// lanes of a wave are added in a xor butterfly (every lane ends with the same bits), the four waves in wave order through
// LDS; rigid_moments_finish_kernel adds the chunk partials in ascending chunk order (as pool.hip does).  The products of two
// float32 values are exact in float64, so only the additions round; their order is fixed: two calls give the same bits.  No
// floating-point atomics anywhere.
#include "common.h"

#pragma clang fp contract(off)

namespace osn {

using u64 = unsigned long long;

constexpr int RS_T = 256;                                    // threads of a score workgroup
constexpr int RS_PPL = 4;                                    // pairs a lane keeps in registers
constexpr int RS_PT = RS_T * RS_PPL;                         // pairs of a tile
constexpr int RS_HT = 64;                                    // hypotheses of a tile: one per lane of a wave
constexpr int RM_T = 256;
constexpr int RM_PPL = OSN_RIGID_MOMENTS_CHUNK / RM_T;
static_assert(OSN_RIGID_MOMENTS_CHUNK % RM_T == 0, "a chunk is dealt to 256 lanes");
constexpr int RB_T = 1024;

struct Xf12 {
    float v[12];                                             // R row-major, t
};

// r2 of one pair under one transform: the contract's sequence, one rounding per operator (contraction is off)
__device__ inline float rigid_r2(const float* __restrict__ x, float s0, float s1, float s2, float d0, float d1, float d2) {
    const float x0 = ((x[0] * s0) + (x[1] * s1)) + (x[2] * s2);
    const float x1 = ((x[3] * s0) + (x[4] * s1)) + (x[5] * s2);
    const float x2 = ((x[6] * s0) + (x[7] * s1)) + (x[8] * s2);
    const float e0 = (x0 + x[9]) - d0;
    const float e1 = (x1 + x[10]) - d1;
    const float e2 = (x2 + x[11]) - d2;
    return ((e0 * e0) + (e1 * e1)) + (e2 * e2);
}

// ------------------------------------------------------------------------------------------------ the fit of a triplet
// The frame of a triangle (p0, p1, p2), float64, every operation rounded on its own, in this order:
//   a = p1 - p0, b = p2 - p0, c = p2 - p1                     |v|^2 = ((v0 v0) + (v1 v1)) + (v2 v2), |v| = sqrt(|v|^2)
//   e1 = a / |a|                                              u x v = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0)
//   n = a x b, e3 = n / |n|, e2 = e3 x e1
struct RigidFrame {
    double e[3][3];                                          // e[k] = e_(k+1)
    double nn;                                               // |n|^2
    double la, lb, lc;                                       // the side lengths |a|, |b|, |c|
};

__device__ inline double rigid_dot(const double* u, const double* v) { return ((u[0] * v[0]) + (u[1] * v[1])) + (u[2] * v[2]); }

__device__ inline void rigid_cross(const double* u, const double* v, double* w) {
    w[0] = (u[1] * v[2]) - (u[2] * v[1]);
    w[1] = (u[2] * v[0]) - (u[0] * v[2]);
    w[2] = (u[0] * v[1]) - (u[1] * v[0]);
}

__device__ inline RigidFrame rigid_frame(const double* p0, const double* p1, const double* p2) {
    RigidFrame f;
    double a[3], b[3], c[3], n[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a[i] = p1[i] - p0[i];
        b[i] = p2[i] - p0[i];
        c[i] = p2[i] - p1[i];
    }
    f.la = __builtin_sqrt(rigid_dot(a, a));
    f.lb = __builtin_sqrt(rigid_dot(b, b));
    f.lc = __builtin_sqrt(rigid_dot(c, c));
    rigid_cross(a, b, n);
    f.nn = rigid_dot(n, n);
    const double ln = __builtin_sqrt(f.nn);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        f.e[0][i] = a[i] / f.la;
        f.e[2][i] = n[i] / ln;
    }
    rigid_cross(f.e[2], f.e[0], f.e[1]);
    return f;
}

// one lane per hypothesis.  R_ij = ((e1d_i e1s_j) + (e2d_i e2s_j)) + (e3d_i e3s_j);  t_i = d0_i - (((R_i0 s0_0) + (R_i1 s0_1))
// + (R_i2 s0_2)) with the float64 R; both rounded to float32 once, at the store.
__global__ __launch_bounds__(256) void rigid_from_triplets_kernel(const float* __restrict__ src, const float* __restrict__ dst, int64_t P,
                                                                  const int32_t* __restrict__ triplets, int H, double thr2,
                                                                  double area2_min, float* __restrict__ xf,
                                                                  uint8_t* __restrict__ valid) {
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= H) return;
    const int64_t i0 = triplets[3 * int64_t(h)], i1 = triplets[3 * int64_t(h) + 1], i2 = triplets[3 * int64_t(h) + 2];
    bool ok = i0 >= 0 && i0 < P && i1 >= 0 && i1 < P && i2 >= 0 && i2 < P && i0 != i1 && i0 != i2 && i1 != i2;
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
    if (ok) {
        double s[3][3], d[3][3];
        const int64_t ix[3] = {i0, i1, i2};
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                s[k][i] = double(src[3 * ix[k] + i]);
                d[k][i] = double(dst[3 * ix[k] + i]);
            }
        const RigidFrame fs = rigid_frame(s[0], s[1], s[2]), fd = rigid_frame(d[0], d[1], d[2]);
        ok = fs.nn > area2_min && fd.nn > area2_min;         // (NaN fails)
        ok = ok && __builtin_fabs(fs.la - fd.la) <= thr2 && __builtin_fabs(fs.lb - fd.lb) <= thr2 && __builtin_fabs(fs.lc - fd.lc) <= thr2;
        if (ok) {
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    R[3 * i + j] = ((fd.e[0][i] * fs.e[0][j]) + (fd.e[1][i] * fs.e[1][j])) + (fd.e[2][i] * fs.e[2][j]);
#pragma unroll
            for (int i = 0; i < 3; ++i)
                t[i] = d[0][i] - (((R[3 * i] * s[0][0]) + (R[3 * i + 1] * s[0][1])) + (R[3 * i + 2] * s[0][2]));
        }
    }
    float* o = xf + 12 * int64_t(h);
#pragma unroll
    for (int i = 0; i < 9; ++i) o[i] = float(R[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) o[9 + i] = float(t[i]);
    valid[h] = ok ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------ the score
__global__ __launch_bounds__(256) void rigid_counts_init_kernel(const uint8_t* __restrict__ valid, int H, int32_t* __restrict__ counts) {
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h < H) counts[h] = (!valid || valid[h]) ? 0 : -1;
}

__global__ __launch_bounds__(RS_T) void rigid_score_kernel(const float* __restrict__ src, const float* __restrict__ dst, int64_t P,
                                                           const float* __restrict__ xf, const uint8_t* __restrict__ valid, int H,
                                                           float tau2, int32_t* __restrict__ counts) {
    __shared__ __attribute__((aligned(16))) float sx[RS_HT][12];
    __shared__ int sok[RS_HT];
    __shared__ int scnt[RS_HT];
    const int tid = threadIdx.x, lane = tid & 63;
    const int h0 = blockIdx.y * RS_HT;
    const int nh = H - h0 < RS_HT ? H - h0 : RS_HT;
    for (int i = tid; i < nh * 12; i += RS_T) (&sx[0][0])[i] = xf[int64_t(h0) * 12 + i];
    if (tid < RS_HT) {
        sok[tid] = tid < nh && (!valid || valid[h0 + tid]);
        scnt[tid] = 0;
    }
    float s[RS_PPL][3], d[RS_PPL][3];
    const float nan = __uint_as_float(0x7FC00000u);
#pragma unroll
    for (int j = 0; j < RS_PPL; ++j) {
        const int64_t p = int64_t(blockIdx.x) * RS_PT + j * RS_T + tid;
        const bool in = p < P;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            s[j][i] = in ? src[3 * p + i] : nan;
            d[j][i] = in ? dst[3 * p + i] : nan;
        }
    }
    __syncthreads();
    int mine = 0;                                            // this wave's count of hypothesis h0 + lane
    for (int hh = 0; hh < nh; ++hh) {
        if (!sok[hh]) continue;                              // (uniform over the workgroup)
        float x[12];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(&sx[hh][4 * q]);
            x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
        }
        int c = 0;
#pragma unroll
        for (int j = 0; j < RS_PPL; ++j) {
            const float r2 = rigid_r2(x, s[j][0], s[j][1], s[j][2], d[j][0], d[j][1], d[j][2]);
            c += __popcll(__ballot(r2 <= tau2));             // (NaN fails)
        }
        if (lane == hh) mine = c;
    }
    if (mine) atomicAdd(&scnt[lane], mine);
    __syncthreads();
    if (tid < nh && scnt[tid]) atomicAdd(counts + h0 + tid, scnt[tid]);
}

// ------------------------------------------------------------------------------------------------------------- the best
// key = (count with its sign bit flipped) << 32 | ~h: the largest key is the largest count and, among equals, the lowest h
__global__ __launch_bounds__(RB_T) void rigid_best_kernel(const int32_t* __restrict__ counts, int H, int32_t* __restrict__ best) {
    __shared__ u64 part[RB_T / 64];
    const int tid = threadIdx.x;
    u64 key = 0;
    for (int h = tid; h < H; h += RB_T) {
        const u64 k = (u64(uint32_t(counts[h]) ^ 0x80000000u) << 32) | u64(~uint32_t(h));
        key = k > key ? k : key;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const u64 o = __shfl_xor(key, m, 64);
        key = o > key ? o : key;
    }
    if ((tid & 63) == 0) part[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < RB_T / 64; ++w) key = part[w] > key ? part[w] : key;
        best[0] = int32_t(uint32_t(key >> 32) ^ 0x80000000u);
        best[1] = int32_t(~uint32_t(key));
    }
}

// ---------------------------------------------------------------------------------------------------------- the moments
constexpr int RM_N = 16;                                     // n, sum s (3), sum d (3), sum s d^T (9, row-major: s_i d_j)

__global__ __launch_bounds__(RM_T) void rigid_moments_kernel(const float* __restrict__ src, const float* __restrict__ dst,
                                                             const int32_t* __restrict__ dst_idx, int64_t P, int64_t n_dst, Xf12 x,
                                                             float tau2, uint8_t* __restrict__ inlier, float* __restrict__ r2out,
                                                             double* __restrict__ partial) {
    __shared__ double part[RM_T / 64][RM_N];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double acc[RM_N];
#pragma unroll
    for (int k = 0; k < RM_N; ++k) acc[k] = 0.0;
#pragma unroll
    for (int j = 0; j < RM_PPL; ++j) {
        const int64_t i = int64_t(blockIdx.x) * OSN_RIGID_MOMENTS_CHUNK + j * RM_T + tid;
        if (i >= P) continue;
        const int64_t q = dst_idx ? int64_t(dst_idx[i]) : i;
        const bool has = q >= 0 && q < n_dst;                // (no partner: never dereferenced)
        float r2 = __uint_as_float(0x7F800000u);
        bool in = false;
        if (has) {
            const float s0 = src[3 * i], s1 = src[3 * i + 1], s2 = src[3 * i + 2];
            const float d0 = dst[3 * q], d1 = dst[3 * q + 1], d2 = dst[3 * q + 2];
            r2 = rigid_r2(x.v, s0, s1, s2, d0, d1, d2);
            in = r2 <= tau2;                                 // (NaN fails)
            if (in) {
                const double s[3] = {double(s0), double(s1), double(s2)}, d[3] = {double(d0), double(d1), double(d2)};
                acc[0] = acc[0] + 1.0;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    acc[1 + a] = acc[1 + a] + s[a];
                    acc[4 + a] = acc[4 + a] + d[a];
#pragma unroll
                    for (int b = 0; b < 3; ++b) acc[7 + 3 * a + b] = acc[7 + 3 * a + b] + (s[a] * d[b]);     // (the product is exact)
                }
            }
        }
        inlier[i] = in ? 1 : 0;
        r2out[i] = r2;
    }
#pragma unroll
    for (int k = 0; k < RM_N; ++k) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc[k] = acc[k] + __shfl_xor(acc[k], m, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < RM_N; ++k) part[wave][k] = acc[k];
    }
    __syncthreads();
    if (tid < RM_N) partial[int64_t(blockIdx.x) * RM_N + tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
}

// one lane per moment: the chunk partials in ascending chunk order, eight loads in flight
__global__ __launch_bounds__(64) void rigid_moments_finish_kernel(const double* __restrict__ partial, int64_t n_chunks,
                                                                  double* __restrict__ moments) {
    const int k = threadIdx.x;
    if (k >= RM_N) return;
    double sum = 0.0;
    int64_t c = 0;
    for (; c + 8 <= n_chunks; c += 8) {
        double t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = partial[(c + j) * RM_N + k];
#pragma unroll
        for (int j = 0; j < 8; ++j) sum = sum + t[j];
    }
    for (; c < n_chunks; ++c) sum = sum + partial[c * RM_N + k];
    moments[k] = sum;
}

static bool finite_nonneg(double v) { return v >= 0.0 && v - v == 0.0; }

}  // namespace osn

using namespace osn;

extern "C" int osn_rigid_from_triplets(const float* src, const float* dst, int64_t n_pairs, const int32_t* triplets, int n_hyp,
                                       float threshold, double area2_min, float* xf, uint8_t* valid, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(n_pairs >= 0 && n_pairs < (int64_t(1) << 31) && n_hyp >= 0 && n_hyp <= OSN_RIGID_MAX_HYPOTHESES, OSN_E_ARG,
                "osn_rigid_from_triplets: n_pairs=%lld (0 .. 2^31 - 1) n_hyp=%d (0 .. %d)", (long long)n_pairs, n_hyp,
                OSN_RIGID_MAX_HYPOTHESES);
    OSN_REQUIRE(finite_nonneg(threshold) && finite_nonneg(area2_min), OSN_E_ARG,
                "osn_rigid_from_triplets: threshold and area2_min must be finite and >= 0");
    if (n_hyp == 0) return OSN_OK;
    OSN_REQUIRE(triplets && xf && valid && (n_pairs == 0 || (src && dst)), OSN_E_ARG, "osn_rigid_from_triplets: null pointer");
    hipLaunchKernelGGL(rigid_from_triplets_kernel, dim3(unsigned(cdiv(n_hyp, 256))), dim3(256), 0, st, src, dst, n_pairs, triplets,
                       n_hyp, 2.0 * double(threshold), area2_min, xf, valid);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_rigid_score(const float* src, const float* dst, int64_t n_pairs, const float* xf, const uint8_t* valid, int n_hyp,
                               float tau2, int32_t* counts, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(n_pairs >= 0 && n_pairs < (int64_t(1) << 31) && n_hyp >= 0 && n_hyp <= OSN_RIGID_MAX_HYPOTHESES, OSN_E_ARG,
                "osn_rigid_score: n_pairs=%lld (0 .. 2^31 - 1) n_hyp=%d (0 .. %d)", (long long)n_pairs, n_hyp, OSN_RIGID_MAX_HYPOTHESES);
    OSN_REQUIRE(finite_nonneg(tau2), OSN_E_ARG, "osn_rigid_score: tau2 must be finite and >= 0");
    if (n_hyp == 0) return OSN_OK;
    OSN_REQUIRE(xf && counts && aligned16(xf) && (n_pairs == 0 || (src && dst)), OSN_E_ARG,
                "osn_rigid_score: null pointer, or xf not 16-byte aligned");
    hipLaunchKernelGGL(rigid_counts_init_kernel, dim3(unsigned(cdiv(n_hyp, 256))), dim3(256), 0, st, valid, n_hyp, counts);
    if (n_pairs > 0) {
        const dim3 grid(unsigned(cdiv(n_pairs, RS_PT)), unsigned(cdiv(n_hyp, RS_HT)));
        hipLaunchKernelGGL(rigid_score_kernel, grid, dim3(RS_T), 0, st, src, dst, n_pairs, xf, valid, n_hyp, tau2, counts);
    }
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_rigid_best(const int32_t* counts, int n_hyp, int32_t* best, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(n_hyp >= 1 && n_hyp <= OSN_RIGID_MAX_HYPOTHESES, OSN_E_ARG, "osn_rigid_best: n_hyp=%d outside 1 .. %d", n_hyp,
                OSN_RIGID_MAX_HYPOTHESES);
    OSN_REQUIRE(counts && best, OSN_E_ARG, "osn_rigid_best: null pointer");
    hipLaunchKernelGGL(rigid_best_kernel, dim3(1), dim3(RB_T), 0, st, counts, n_hyp, best);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" size_t osn_rigid_moments_ws_bytes(int64_t n_pairs) {
    const int64_t chunks = n_pairs > 0 ? cdiv(n_pairs, OSN_RIGID_MOMENTS_CHUNK) : 0;
    return align_up(size_t(chunks > 0 ? chunks : 1) * RM_N * sizeof(double), 256);
}

extern "C" int osn_rigid_moments(const float* src, const float* dst, const int32_t* dst_idx, int64_t n_pairs, int64_t n_dst,
                                 const float* xf12_host, float tau2, uint8_t* inlier, float* r2, double* moments, void* ws,
                                 size_t ws_bytes, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t lim = int64_t(1) << 31;
    OSN_REQUIRE(n_pairs >= 0 && n_pairs < lim && n_dst >= 0 && n_dst < lim, OSN_E_ARG,
                "osn_rigid_moments: n_pairs=%lld n_dst=%lld (0 .. 2^31 - 1)", (long long)n_pairs, (long long)n_dst);
    OSN_REQUIRE(dst_idx || n_dst >= n_pairs, OSN_E_ARG, "osn_rigid_moments: without dst_idx dst holds a row per pair (n_dst=%lld < %lld)",
                (long long)n_dst, (long long)n_pairs);
    OSN_REQUIRE(finite_nonneg(tau2), OSN_E_ARG, "osn_rigid_moments: tau2 must be finite and >= 0");
    OSN_REQUIRE(xf12_host && moments, OSN_E_ARG, "osn_rigid_moments: null pointer");
    OSN_REQUIRE(n_pairs == 0 || (src && inlier && r2 && (n_dst == 0 || dst)), OSN_E_ARG, "osn_rigid_moments: null pointer");
    const size_t need = osn_rigid_moments_ws_bytes(n_pairs);
    OSN_REQUIRE(ws && aligned16(ws) && ws_bytes >= need, OSN_E_WS, "osn_rigid_moments: workspace too small (%zu < %zu)", ws_bytes, need);
    Xf12 x;
    for (int i = 0; i < 12; ++i) x.v[i] = xf12_host[i];
    double* partial = static_cast<double*>(ws);
    const int64_t chunks = cdiv(n_pairs, OSN_RIGID_MOMENTS_CHUNK);
    if (chunks > 0)
        hipLaunchKernelGGL(rigid_moments_kernel, dim3(unsigned(chunks)), dim3(RM_T), 0, st, src, dst, dst_idx, n_pairs, n_dst, x, tau2,
                           inlier, r2, partial);
    hipLaunchKernelGGL(rigid_moments_finish_kernel, dim3(1), dim3(64), 0, st, partial, chunks, moments);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}
