// Evaluation-mode batch norm (+ residual) (+ ReLU) (+ second store) in the epilogue of the kernel that produces a convolution's final
// rows (round 6; the network executor's inference pass, net.hip).
//
// models/mink_unet.py:126-172 / models/resnet_base.py:92-118 follow every convolution but the last with a batch norm; in evaluation mode
// that is a per-column affine map of the finished row -- a second launch that reads the convolution's output and writes it again
// (48 launches, 0.40 of 4.0 ms of kernel time of a MinkUNet18A inference pass on 101 k voxels: profiles/r06_s7_*).  Every kernel
// below holds the finished fp32 value in a register right before its store, so it applies
//     y = relu(bn_val(x, mean, 1 / sqrt(var + eps), gamma, beta) + residual)
// there, with the SAME expression in the same order as bn_apply_kernel (bn.hip): the result is bitwise the two-launch path's (and
// therefore the module-by-module path's, functional.py).  Training keeps the separate launches: batch statistics need every row first.
#pragma once
#include "common.h"

namespace osn {

// The normalised value, ONE definition for the forward kernels, the epilogues and the backward kernels that recompute the ReLU mask
// from x instead of reading y (round 4): explicit fma so that every side rounds identically whatever the surrounding code.
__device__ inline float bn_val(float x, float mu, float is, float ga, float be) { return __fmaf_rn((x - mu) * is, ga, be); }
__device__ inline float bn_is(float var, float eps) { return 1.f / sqrtf(var + eps); }
// The ReLU behind a batch norm, ONE definition like bn_val: a NaN propagates as torch.relu does (fmaxf(x, 0.f) returns 0 for a NaN,
// and a diverged run would go on training on zeros); every finite or infinite x gives the bits fmaxf gave.
__device__ inline float bn_relu(float x) { return x > 0.f ? x : (x != x ? x : 0.f); }

struct Epi {
    const float* mean;      // nullptr: no epilogue, the plain convolution result is stored
    const float* var;
    const float* gamma;
    const float* beta;
    const float* res;       // residual rows [n_out, cout] in the OUTPUT's row order, or nullptr
    float* y2;              // second store (ME.cat written in place): rows of pitch ld2, first column already applied; or nullptr
    int64_t ld2;
    float eps;
    int relu;
};

inline Epi epi_none() { return Epi{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0.f, 0}; }

// The per-column constants of four consecutive columns (a thread that stores several rows of the same columns loads them and takes the
// four reciprocal square roots ONCE: bn_is is a pure function of (var, eps), so where it is evaluated does not change a bit)
struct EpiCols {
    float4 mu, is, ga, be;
};
__device__ inline float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ inline EpiCols epi_cols(const float* mean, const float* var, const float* gamma, const float* beta, float eps, int col) {
    EpiCols c;
    c.mu = ld4(mean + col);
    const float4 vv = ld4(var + col);
    c.is = make_float4(bn_is(vv.x, eps), bn_is(vv.y, eps), bn_is(vv.z, eps), bn_is(vv.w, eps));
    c.ga = ld4(gamma + col);
    c.be = ld4(beta + col);
    return c;
}
__device__ inline EpiCols epi_cols(const Epi& e, int col) { return epi_cols(e.mean, e.var, e.gamma, e.beta, e.eps, col); }

// The forward quad, ONE definition for the three forward kernels of bn.hip: normalise, add the residual quad, clamp.  res() gives the
// residual quad and is called only with has_res: a caller loads it there (behind the branch) or hands over a quad it loaded ahead.
template <class Res>
__device__ inline float4 bn_fwd_quad(float4 x, const EpiCols& c, bool has_res, Res res, int relu) {
    float4 o;
    o.x = bn_val(x.x, c.mu.x, c.is.x, c.ga.x, c.be.x);
    o.y = bn_val(x.y, c.mu.y, c.is.y, c.ga.y, c.be.y);
    o.z = bn_val(x.z, c.mu.z, c.is.z, c.ga.z, c.be.z);
    o.w = bn_val(x.w, c.mu.w, c.is.w, c.ga.w, c.be.w);
    if (has_res) {
        const float4 rv = res();
        o.x += rv.x; o.y += rv.y; o.z += rv.z; o.w += rv.w;
    }
    if (relu) {
        o.x = bn_relu(o.x); o.y = bn_relu(o.y); o.z = bn_relu(o.z); o.w = bn_relu(o.w);
    }
    return o;
}

// The gradient at a batch norm's pre-activation, ONE definition for the column sums and the backward apply passes: the sum of the
// n_src loaded source quads, source 0 first, under the ReLU mask -- none (no relu), from y, or (from_x) from x through the forward
// expression (bn_val with the constants c: bit for bit the y > 0 of a norm without a residual).  x, y and c are read only under their
// mask: they may be unset.  No contraction pragma here: nothing to contract.
template <int N>
__device__ inline float4 bn_masked_grad(const float4 (&gs)[N], int n_src, const float4& x, const float4& y, const EpiCols& c,
                                        bool relu, bool from_x) {
    float4 g = gs[0];
#pragma unroll
    for (int i = 1; i < N; ++i)
        if (i < n_src) { g.x += gs[i].x; g.y += gs[i].y; g.z += gs[i].z; g.w += gs[i].w; }
    if (from_x) {
        g.x = bn_val(x.x, c.mu.x, c.is.x, c.ga.x, c.be.x) > 0.f ? g.x : 0.f;
        g.y = bn_val(x.y, c.mu.y, c.is.y, c.ga.y, c.be.y) > 0.f ? g.y : 0.f;
        g.z = bn_val(x.z, c.mu.z, c.is.z, c.ga.z, c.be.z) > 0.f ? g.z : 0.f;
        g.w = bn_val(x.w, c.mu.w, c.is.w, c.ga.w, c.be.w) > 0.f ? g.w : 0.f;
    } else if (relu) {
        g.x = y.x > 0.f ? g.x : 0.f; g.y = y.y > 0.f ? g.y : 0.f;
        g.z = y.z > 0.f ? g.z : 0.f; g.w = y.w > 0.f ? g.w : 0.f;
    }
    return g;
}

// The column constants of a backward apply pass, each taken only where it is used: mean with batch statistics or the mask from x,
// beta with the mask from x, the two column sums with batch statistics.  gi = ga * is: the output's  ga * is * (...)  is
// (ga * is) * (...), and bn_is is a pure function, so forming gi once per thread or once per quad gives the same bits.
struct BnBwdCols {
    EpiCols c;
    float4 gi, sg, sx;
};
// (sum_col: where column `col` stands in sum_g / sum_gx -- `col` itself, or its place in a workgroup's own totals)
__device__ inline BnBwdCols bn_bwd_cols(const float* mean, const float* var, const float* gamma, const float* beta, const float* sum_g,
                                        const float* sum_gx, float eps, bool training, bool from_x, int col, int sum_col) {
    const float4 z = make_float4(0, 0, 0, 0), vv = ld4(var + col);
    BnBwdCols k;
    k.c.is = make_float4(bn_is(vv.x, eps), bn_is(vv.y, eps), bn_is(vv.z, eps), bn_is(vv.w, eps));
    k.c.ga = ld4(gamma + col);
    k.c.mu = (training || from_x) ? ld4(mean + col) : z;
    k.c.be = from_x ? ld4(beta + col) : z;
    k.sg = training ? ld4(sum_g + sum_col) : z;
    k.sx = training ? ld4(sum_gx + sum_col) : z;
    k.gi = make_float4(k.c.ga.x * k.c.is.x, k.c.ga.y * k.c.is.y, k.c.ga.z * k.c.is.z, k.c.ga.w * k.c.is.w);
    return k;
}

// The backward output quad, ONE definition:  ga * is * (g - sg / n - xhat * sx / n)  with batch statistics,  ga * is * g  without.
// Contraction is off INSIDE this function (a helper keeps the setting of the scope it is written in, wherever it is inlined) and the
// two fused steps are written, so no batch-norm output depends on what the compiler chooses to contract.
__device__ inline float4 bn_bwd_quad(float4 g, float4 x, const BnBwdCols& k, float inv_n, int training) {
#pragma clang fp contract(off)
    float4 o;
    if (training) {
        o.x = k.gi.x * __fmaf_rn(-((x.x - k.c.mu.x) * k.c.is.x * k.sx.x), inv_n, __fmaf_rn(-k.sg.x, inv_n, g.x));
        o.y = k.gi.y * __fmaf_rn(-((x.y - k.c.mu.y) * k.c.is.y * k.sx.y), inv_n, __fmaf_rn(-k.sg.y, inv_n, g.y));
        o.z = k.gi.z * __fmaf_rn(-((x.z - k.c.mu.z) * k.c.is.z * k.sx.z), inv_n, __fmaf_rn(-k.sg.z, inv_n, g.z));
        o.w = k.gi.w * __fmaf_rn(-((x.w - k.c.mu.w) * k.c.is.w * k.sx.w), inv_n, __fmaf_rn(-k.sg.w, inv_n, g.w));
    } else {
        o.x = k.gi.x * g.x; o.y = k.gi.y * g.y; o.z = k.gi.z * g.z; o.w = k.gi.w * g.w;
    }
    return o;
}

// columns col .. col + 3 of output row `row` (row pitch cout for the residual): normalise, add, clamp, second store; returns the quad to store.
// The one remaining SECOND COPY of bn_fwd_quad's text: written through bn_fwd_quad -- the residual loaded ahead, handed over as a
// pointer, or loaded by a callable inside the helper -- at least one convolution kernel compiles to another instruction order, and
// their ISA is to stay what it was.  Keep the two in step (tests/test_gpu_unet.py compares the two paths bit for bit).
__device__ inline float4 epi_apply(const Epi& e, const EpiCols& c, float4 x, int64_t row, int col, int cout) {
    float4 o;
    o.x = bn_val(x.x, c.mu.x, c.is.x, c.ga.x, c.be.x);
    o.y = bn_val(x.y, c.mu.y, c.is.y, c.ga.y, c.be.y);
    o.z = bn_val(x.z, c.mu.z, c.is.z, c.ga.z, c.be.z);
    o.w = bn_val(x.w, c.mu.w, c.is.w, c.ga.w, c.be.w);
    if (e.res) {
        const float4 rv = *reinterpret_cast<const float4*>(e.res + row * cout + col);
        o.x += rv.x; o.y += rv.y; o.z += rv.z; o.w += rv.w;
    }
    if (e.relu) {
        o.x = bn_relu(o.x); o.y = bn_relu(o.y); o.z = bn_relu(o.z); o.w = bn_relu(o.w);
    }
    if (e.y2) *reinterpret_cast<float4*>(e.y2 + row * e.ld2 + col) = o;
    return o;
}
__device__ inline float4 epi_quad(const Epi& e, float4 x, int64_t row, int col, int cout) {
    return epi_apply(e, epi_cols(e, col), x, row, col, cout);
}

// ---- the library's convolution launches with an epilogue (net.hip); the extern "C" entry points pass epi_none().
// pieces (split.h): 3 = the six-product arithmetic, 2 / 1 = the reduced inference modes of the four split-bf16 forward families
int spconv_fwd_tl_epi(const float* in, int64_t n_in, const void* Wp, const void* tl, const int32_t* out_rows, float* out, int64_t n_out,
                      int K, int cin, int cout, int bm, void* ws, size_t ws_bytes, int32_t* counters, const Epi& epi, osn_stream_t stream,
                      int pieces = 3);
int spconv_fwd_ws_epi(const float* in, int64_t n_in, const void* Wp, const void* pl, int64_t pl_rows, int swap, int direct,
                      const int32_t* nbr_dst, float* out, int64_t n_dst, int K, int cin, int cout, void* ws, size_t ws_bytes, const Epi& epi,
                      osn_stream_t stream, int pieces = 3);
int spconv_fwd_rg_epi(const float* in, int64_t n_in, const void* Wp, const int32_t* nbr, const int32_t* out_rows, float* out,
                      int64_t n_out, int K, int cin, int cout, const Epi& epi, osn_stream_t stream, int pieces = 3);
int dense_fwd_epi(const float* in, const void* Wp, float* out, int64_t n, int cin, int cout, const Epi& epi, osn_stream_t stream,
                  int pieces = 3);
int stem_conv_fwd_epi(const float* in, const float* W, const int32_t* nbr, float* out, int64_t n_out, int K, int cin, int cout,
                      const Epi& epi, osn_stream_t stream);

}  // namespace osn
