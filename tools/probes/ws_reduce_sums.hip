// Probe (tools/micro_ws_sums.py; not part of the library): the gate of "the weight-stationary reduction emits the next norm's backward
// column sums".  One translation unit with the library's own kernels, so that the separate chain below IS the product's:
//   separate  spconv_ws_reduce_kernel<KT>  ->  col_reduce_kernel<1, MASK>   (one gradient source: the reduction's output)
//   fused     ws_reduce_sums_kernel<KT, MASK>: col_reduce_body's geometry -- block (row block, 64-column group), thread (row lane,
//             column quad), rows r, r + 16, ... in order, fp64 sums, row lanes combined in the fixed order -- whose row is the
//             ascending-k sum over the partial planes (the adds of spconv_ws_reduce_kernel), stored as the finished row.
// Both write the finished rows and the [n_rb][2][c] fp64 partials; the tool compares them bit for bit and times them.
#include "../../openscene_amd/csrc/bn.hip"
#include "../../openscene_amd/csrc/spconv_ws.hip"

namespace osn {

// WAVES: waves per SIMD the instance is held to (4: at most 128 VGPRs; 8: at most 64, the budget beside wgrad_tl_kernel<4,4>)
template <int KT, int MASK, int WAVES>
__global__ __launch_bounds__(256, WAVES) void ws_reduce_sums_kernel(const float* __restrict__ planes, const int32_t* __restrict__ nbr,
                                                             const float* __restrict__ zeros, float* __restrict__ out, int64_t n, int c,
                                                             const float* __restrict__ x, const float* __restrict__ mean,
                                                             const float* __restrict__ var, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps, int rows_per_block,
                                                             double* __restrict__ partial) {
    __shared__ double red[2][CR_RL][CR_COLS];
    constexpr int G = KT % WS_RED_GROUP == 0 ? WS_RED_GROUP : KT;
    const int tid = threadIdx.x, cl = tid & 15, rl = tid >> 4;
    const int col = blockIdx.y * CR_COLS + cl * 4;
    const bool on = col < c;
    const int64_t r0 = int64_t(blockIdx.x) * rows_per_block, r1 = min(n, r0 + rows_per_block);
    double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    const float4 z = make_float4(0, 0, 0, 0);
    EpiCols k{z, z, z, z};
    constexpr bool from_x = MASK == CR_MASK_X, masked = MASK != CR_MASK_NONE;
    if (on) {
        k.mu = ld4(mean + col);
        const float4 v = ld4(var + col);
        k.is = make_float4(bn_is(v.x, eps), bn_is(v.y, eps), bn_is(v.z, eps), bn_is(v.w, eps));
        if (from_x) { k.ga = ld4(gamma + col); k.be = ld4(beta + col); }
        for (int64_t r = r0 + rl; r < r1; r += CR_RL) {
            const float4 xv = ld4(x + r * c + col);
            unsigned present = 0;
#pragma unroll
            for (int kk = 0; kk < KT; ++kk) present |= (nbr[int64_t(kk) * n + r] >= 0 ? 1u : 0u) << kk;
            float4 s = z;
#pragma unroll 1
            for (int k0 = 0; k0 < KT; k0 += G) {
                float4 v[G];
#pragma unroll
                for (int j = 0; j < G; ++j) v[j] = ld4((present >> (k0 + j)) & 1u ? planes + (int64_t(k0 + j) * n + r) * c + col : zeros);
#pragma unroll
                for (int j = 0; j < G; ++j) { s.x += v[j].x; s.y += v[j].y; s.z += v[j].z; s.w += v[j].w; }
            }
            *reinterpret_cast<float4*>(out + r * c + col) = s;
            const float4 gs[1] = {s};
            const float4 g = bn_masked_grad(gs, 1, xv, z, k, masked, from_x);
            s1[0] += g.x; s1[1] += g.y; s1[2] += g.z; s1[3] += g.w;
            s2[0] += double(g.x) * ((xv.x - k.mu.x) * k.is.x); s2[1] += double(g.y) * ((xv.y - k.mu.y) * k.is.y);
            s2[2] += double(g.z) * ((xv.z - k.mu.z) * k.is.z); s2[3] += double(g.w) * ((xv.w - k.mu.w) * k.is.w);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        red[0][rl][cl * 4 + j] = s1[j];
        red[1][rl][cl * 4 + j] = s2[j];
    }
    __syncthreads();
    if (tid < 2 * CR_COLS) {
        const int which = tid / CR_COLS, cc = tid % CR_COLS;
        double s = 0;
#pragma unroll
        for (int r = 0; r < CR_RL; ++r) s += red[which][r][cc];
        const int gc = blockIdx.y * CR_COLS + cc;
        if (gc < c) partial[(int64_t(blockIdx.x) * 2 + which) * c + gc] = s;
    }
}

}  // namespace osn

// fused 0: the two launches of the product; 1: the one kernel above within 128 VGPRs; 2: within 64.  K = 27 or 8; mask_x 0: no ReLU, 1: the mask from x.
extern "C" int osn_dbg_ws_reduce_sums(int fused, const float* planes, const int32_t* nbr, const float* zeros, float* out, int64_t n, int K,
                                      int c, const float* x, const float* mean, const float* var, const float* gamma, const float* beta,
                                      float eps, int mask_x, double* partial, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!(K == 27 || K == 8) || n < 1 || c < 4 || (c & 3)) return 1;
    const ColReducePlan p = plan_colreduce(n, c);
    const dim3 sgrid(p.n_rb, p.n_cg);
    if (fused) {
#define OSN_F2(KT_, M_, W_) hipLaunchKernelGGL((ws_reduce_sums_kernel<KT_, M_, W_>), sgrid, dim3(256), 0, st, planes, nbr, zeros, out, n, c, x, mean, var, gamma, beta, eps, p.rows_per_block, partial)
#define OSN_F(KT_, M_) do { if (fused == 2) OSN_F2(KT_, M_, 8); else OSN_F2(KT_, M_, 4); } while (0)
        if (K == 27) { if (mask_x) OSN_F(27, CR_MASK_X); else OSN_F(27, CR_MASK_NONE); }
        else { if (mask_x) OSN_F(8, CR_MASK_X); else OSN_F(8, CR_MASK_NONE); }
#undef OSN_F
#undef OSN_F2
    } else {
        const int c4 = c / 4;
        const dim3 rgrid(unsigned(cdiv(n * c4, 256)));
        if (K == 27) hipLaunchKernelGGL((spconv_ws_reduce_kernel<27, false>), rgrid, dim3(256), 0, st, planes, nbr, zeros, out, n, K, c4, epi_none());
        else hipLaunchKernelGGL((spconv_ws_reduce_kernel<8, false>), rgrid, dim3(256), 0, st, planes, nbr, zeros, out, n, K, c4, epi_none());
        GySrc src{};
        src.n = 1;
        for (int i = 0; i < BN_MAX_SRC; ++i) { src.p[i] = out; src.ld[i] = c; }
        if (mask_x)
            hipLaunchKernelGGL((col_reduce_kernel<1, CR_MASK_X>), sgrid, dim3(256), 0, st, x, (const float*)nullptr, src, mean, var, eps, 1, n, c,
                               p.rows_per_block, partial, gamma, beta);
        else
            hipLaunchKernelGGL((col_reduce_kernel<1, CR_MASK_NONE>), sgrid, dim3(256), 0, st, x, (const float*)nullptr, src, mean, var, eps, 0, n, c,
                               p.rows_per_block, partial, gamma, beta);
    }
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
