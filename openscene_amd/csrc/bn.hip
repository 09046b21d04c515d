// Batch-norm statistics, fused normalise(+residual)(+ReLU), and backward on
// gfx950.  Pure streaming work (HBM-bound): 16-byte loads, lanes along the
// channel axis, fp64 accumulators, deterministic two-stage column reductions
// (per-block partials -> ordered final sum; no floating-point atomics).
//
// Function parity with torch.nn.BatchNorm1d as wrapped by MinkowskiBatchNorm,
// MinkowskiReLU and the BasicBlock residual add.
#include "common.h"
#include "epilogue.h"

#include <atomic>

namespace osn {

constexpr int CR_COLS = 64;    // columns per block (16 lanes x float4)
constexpr int CR_RL = 16;      // row lanes per block
constexpr int CR_MAX_BLOCKS = 512;

// The gradient arriving at a batch norm's output may be the SUM of several row-aligned matrices (a block input feeds
// conv1 and the residual; an encoder output feeds the next stride-2 conv and, through ME.cat, two convs of the decoder --
// models/mink_unet.py:116-174), each possibly a column window of a wider matrix (ld = row stride in floats).  The
// backward kernels add them while they read: no separate accumulation pass, no torch add.
constexpr int BN_MAX_SRC = 3;
struct GySrc {
    const float* p[BN_MAX_SRC];
    int64_t ld[BN_MAX_SRC];
    int n;
};

// the source quads of (row r, columns col .. col + 3) as they arrive; bn_masked_grad (epilogue.h) adds them
template <int N>
__device__ __forceinline__ void gy_load(float4 (&g)[N], const GySrc& s, int64_t r, int col) {
    g[0] = ld4(s.p[0] + r * s.ld[0] + col);
#pragma unroll
    for (int i = 1; i < N; ++i)
        if (i < s.n) g[i] = ld4(s.p[i] + r * s.ld[i] + col);
}

struct ColReducePlan {
    int n_rb;            // row blocks
    int n_cg;            // column groups
    int rows_per_block;
};

static ColReducePlan plan_colreduce(int64_t n, int c) {
    ColReducePlan p;
    p.n_cg = int(cdiv(c, CR_COLS));
    int64_t rb = cdiv(n, 4 * CR_RL);
    if (rb > CR_MAX_BLOCKS) rb = CR_MAX_BLOCKS;
    if (rb < 1) rb = 1;
    p.rows_per_block = int(cdiv(cdiv(n, rb), CR_RL) * CR_RL);
    p.n_rb = int(cdiv(n, p.rows_per_block));
    if (p.n_rb < 1) p.n_rb = 1;
    return p;
}

// Rows a thread of the column sums keeps IN FLIGHT (its rows r, r + 16, ...: all their loads are issued before the first add).
// With one row per thread a CU holds ~16 KB of loads and the kernel runs at a third of the HBM roof, for as long as the loaded
// latency -- which the weight-gradient stream beside it raises.  Per instance: a row costs one quad of
// VGPRs in the statistics pass and 2 - 5 (x, the sources, y) in the backward passes.  1 = the loop of the earlier rounds.
#ifndef OSN_BN_ROWS_STATS
#define OSN_BN_ROWS_STATS 4
#endif

// The backward sums run on the main stream BESIDE the weight gradients of the side stream, whose two waves per SIMD hold 320 - 448
// of a SIMD's 512 VGPRs for a whole launch: a column sum gets the waves that fit into the rest, so the
// backward sums without a gres store stay within CR_BWD_VGPRS registers (those with the store: col_reduce_gres_kernel below).
// What a launch does not use is chosen at compile time -- a register that an `if (i < n)` load MAY fill is allocated for every launch:
//   MASK  none (no ReLU), from x (ReLU, no residual: gamma and beta are read, y is not), from y -- one kernel each, picked by the
//         host (osn_bn_backward); CR_MASK_RT: read from the arguments at run time (the one-row kernels of
//         osn_bn_set_flat_kernels)
//   NSRC  1: one gradient source; BN_MAX_SRC: gy.n of them, as before; CR_SRC_BRANCH: both row loops in one kernel, chosen by a
//         uniform branch on gy.n (a kernel's name and grid then say nothing about how many matrices its gradient arrives in: the
//         module path adds them beforehand, the executor hands them over, and both launch the same kernels)
constexpr int CR_BWD_VGPRS = 64;
constexpr int CR_MASK_NONE = 0, CR_MASK_X = 1, CR_MASK_Y = 2, CR_MASK_RT = 3;
constexpr int CR_SRC_BRANCH = 0;

// Rows in flight of a backward instance.  Two fit in CR_BWD_VGPRS registers where there is one source (60 - 64, no scratch), and
// measured beside the weight gradient they lose to one: a level-0 backward takes 66.5 us with two rows against 57.9 us with one
// beside wgrad_tl_kernel<3,3>, 89 against 78 us beside <4,3> (profiles/r25_backward_light_kernels_gate.txt).  With one row the
// one-source loops hold at most 56 registers.  OSN_BN_ROWS_BWD (1 or 2, an A/B build): the rows of the one-source loops where two fit.
#ifndef OSN_BN_ROWS_BWD
#define OSN_BN_ROWS_BWD 1
#endif
constexpr int cr_bwd_rows(int mask) {
    return mask != CR_MASK_Y ? OSN_BN_ROWS_BWD : 1;          // (mask from y: two rows spill)
}
template <int V>
struct CrInt {
    static constexpr int value = V;
};

// one row's operands as they arrive (the sources are added afterwards, source 0 first)
template <int NSRC>
struct CrRow {
    float4 x, y, g[NSRC];
};

template <int MODE, int NSRC>
__device__ __forceinline__ void cr_load(CrRow<NSRC>& w, const float* __restrict__ x, const float* __restrict__ y, const GySrc& gy,
                                        bool need_y, int64_t r, int c, int col) {
    w.x = ld4(x + r * c + col);
    if (MODE == 1) {
        gy_load(w.g, gy, r, col);
        if (need_y) w.y = ld4(y + r * c + col);
    }
}

// MODE 0: (sum x, sum x^2)        MODE 1: (sum g, sum g*xhat), g = relu ? gy*(y>0) : gy
// STORE_G (MODE 1, a batch norm with a residual): the masked g this pass already holds is stored as gres -- the value the apply
// pass used to form a second time from y and the sources -- and bn_bwd_apply_gres_kernel reads it back: one read of y and of
// every source less per residual norm.  Every (row, column) is visited by exactly one thread, so gres is written once.
// R rows in flight: the loads of rows r, r + 16, ... r + 16 (R - 1) first, then the adds in row order into the same accumulators
// -- every sum is formed in the order of the one-row loop, bit for bit.  A ragged last round loads its missing rows from row r
// (an address inside the matrix) and does not add them.  (R: the rows of the statistics pass, of the one-source loop, and of the
// run-time loop of the one-row kernels; the loop over gy.n sources of a CR_SRC_BRANCH kernel keeps one.)
template <int MODE, bool STORE_G, int R, int NSRC = BN_MAX_SRC, int MASK = CR_MASK_RT>
__device__ __forceinline__ void col_reduce_body(const float* __restrict__ x, const float* __restrict__ y, const GySrc gy,
                                                const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                                int relu, int64_t n, int c, int rows_per_block, double* __restrict__ partial,
                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                float* __restrict__ gres) {
    static_assert(!STORE_G || MODE == 1, "only the backward sums form g");
    static_assert(R >= 1 && R <= 4, "rows in flight");
    static_assert(NSRC == 1 || NSRC == BN_MAX_SRC || NSRC == CR_SRC_BRANCH, "one source, gy.n of them, or a branch between the two");
    static_assert(MASK != CR_MASK_X || !STORE_G, "a residual's mask is y's");
    __shared__ double red[2][CR_RL][CR_COLS];
    const int tid = threadIdx.x;
    const int cl = tid & 15, rl = tid >> 4;
    const int col = blockIdx.y * CR_COLS + cl * 4;
    const bool on = col < c;
    const int64_t r0 = int64_t(blockIdx.x) * rows_per_block;
    const int64_t r1 = min(n, r0 + rows_per_block);
    double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    const float4 z = make_float4(0, 0, 0, 0);
    EpiCols k{z, z, z, z};
    constexpr bool RT = MASK == CR_MASK_RT;
    const bool from_x = RT ? MODE == 1 && !STORE_G && relu && !y : MASK == CR_MASK_X; // the ReLU mask recomputed from x (no residual): y is not read
    const bool need_y = RT ? MODE == 1 && relu && !from_x : MASK == CR_MASK_Y;
    const bool masked = RT ? relu != 0 : MASK != CR_MASK_NONE;
    if (MODE == 1 && on) {
        k.mu = ld4(mean + col);
        const float4 v = ld4(var + col);
        k.is = make_float4(bn_is(v.x, eps), bn_is(v.y, eps), bn_is(v.z, eps), bn_is(v.w, eps));
        if (from_x) {
            k.ga = ld4(gamma + col);
            k.be = ld4(beta + col);
        }
    }
    auto add_row = [&](const auto& w, int n_src, int64_t r) {
        const float4 xv = w.x;
        if (MODE == 0) {
            s1[0] += xv.x; s1[1] += xv.y; s1[2] += xv.z; s1[3] += xv.w;
            s2[0] += double(xv.x) * xv.x; s2[1] += double(xv.y) * xv.y;
            s2[2] += double(xv.z) * xv.z; s2[3] += double(xv.w) * xv.w;
        } else {
            const float4 g = bn_masked_grad(w.g, n_src, xv, w.y, k, masked, from_x);
            if (STORE_G) *reinterpret_cast<float4*>(gres + r * c + col) = g;
            s1[0] += g.x; s1[1] += g.y; s1[2] += g.z; s1[3] += g.w;
            s2[0] += double(g.x) * ((xv.x - k.mu.x) * k.is.x); s2[1] += double(g.y) * ((xv.y - k.mu.y) * k.is.y);
            s2[2] += double(g.z) * ((xv.z - k.mu.z) * k.is.z); s2[3] += double(g.w) * ((xv.w - k.mu.w) * k.is.w);
        }
    };
    // the row loop over NS sources (1: one; BN_MAX_SRC: gy.n of them), RR rows in flight
    auto rows = [&](auto ns, auto rr) {
        constexpr int NS = decltype(ns)::value, RR = decltype(rr)::value;
        const int n_src = NS == 1 ? 1 : gy.n;
        // (the row inside the block as a 32-bit count: one register for the loop instead of a 64-bit row and its compare)
        const int nr = int(r1 - r0);                         // 1 .. rows_per_block
        int i = rl;
        for (; i + (RR - 1) * CR_RL < nr; i += RR * CR_RL) {
            const int64_t r = r0 + i;
            CrRow<NS> w[RR];
#pragma unroll
            for (int k = 0; k < RR; ++k) cr_load<MODE>(w[k], x, y, gy, need_y, r + k * CR_RL, c, col);
#pragma unroll
            for (int k = 0; k < RR; ++k) add_row(w[k], n_src, r + k * CR_RL);
        }
        if constexpr (RR > 1) {
            if (i < nr) {                                    // ragged last round: 1 .. RR - 1 rows
                const int64_t r = r0 + i;
                CrRow<NS> w[RR - 1];
#pragma unroll
                for (int k = 0; k < RR - 1; ++k)
                    cr_load<MODE>(w[k], x, y, gy, need_y, i + k * CR_RL < nr ? r + k * CR_RL : r, c, col);
#pragma unroll
                for (int k = 0; k < RR - 1; ++k)
                    if (i + k * CR_RL < nr) add_row(w[k], n_src, r + k * CR_RL);
            }
        }
    };
    if (on) {
        if constexpr (NSRC == CR_SRC_BRANCH) {
            if (gy.n == 1) rows(CrInt<1>{}, CrInt<R>{});
            else rows(CrInt<BN_MAX_SRC>{}, CrInt<1>{});
        } else {
            rows(CrInt<NSRC>{}, CrInt<R>{});
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

#define OSN_CR_PARAMS                                                                                                          \
    const float *__restrict__ x, const float *__restrict__ y, const GySrc gy, const float *__restrict__ mean,                    \
        const float *__restrict__ var, float eps, int relu, int64_t n, int c, int rows_per_block, double *__restrict__ partial

// MODE 0: the statistics pass (MASK unused).  MODE 1: one kernel per mask.
template <int MODE, int MASK = CR_MASK_NONE>
__global__ __launch_bounds__(256, 512 / CR_BWD_VGPRS) void col_reduce_kernel(OSN_CR_PARAMS, const float* __restrict__ gamma,
                                                                             const float* __restrict__ beta) {
    col_reduce_body<MODE, false, MODE == 0 ? OSN_BN_ROWS_STATS : cr_bwd_rows(MASK), MODE == 0 ? 1 : CR_SRC_BRANCH, MASK>(
        x, y, gy, mean, var, eps, relu, n, c, rows_per_block, partial, gamma, beta, nullptr);
}

// The sums that store gres keep the loop of round 23 -- every operand a run-time choice, two rows in flight, 106 registers: held to
// CR_BWD_VGPRS with one row in flight (60 - 64 registers, a kernel per mask) they were 9 % SLOWER in the step (0.287 -> 0.312 ms over
// their 16 launches, profiles/r25_backward_light_kernels_ab_steps.txt), where the sums without the store gained 4 %.
#ifndef OSN_BN_ROWS_GRES
#define OSN_BN_ROWS_GRES 2
#endif
__global__ __launch_bounds__(256) void col_reduce_gres_kernel(OSN_CR_PARAMS, float* __restrict__ gres) {
    col_reduce_body<1, true, OSN_BN_ROWS_GRES>(x, y, gy, mean, var, eps, relu, n, c, rows_per_block, partial, nullptr, nullptr, gres);
}

// One row in flight: the loops of the earlier rounds, run by osn_bn_set_flat_kernels(1) (tests, A/B).
template <int MODE>
__global__ __launch_bounds__(256) void col_reduce_1row_kernel(OSN_CR_PARAMS, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta) {
    col_reduce_body<MODE, false, 1>(x, y, gy, mean, var, eps, relu, n, c, rows_per_block, partial, gamma, beta, nullptr);
}

__global__ __launch_bounds__(256) void col_reduce_gres_1row_kernel(OSN_CR_PARAMS, float* __restrict__ gres) {
    col_reduce_body<1, true, 1>(x, y, gy, mean, var, eps, relu, n, c, rows_per_block, partial, nullptr, nullptr, gres);
}

// Final column sums: FIN_COLS columns x FIN_PARTS slices of the partial blocks per workgroup
// (the partial blocks are summed in a fixed order => deterministic).
// FIN_COLS: columns per finalize workgroup (a power of two; x FIN_PARTS slices = its threads).  4: a workgroup of 256 threads, one wave of 48
// registers per SIMD.  With 16 (1024 threads: four waves, 192 registers per SIMD, all placed at once) a backward finalize launch found
// no CU to start on while wgrad_tl_kernel<4,4> held 448 of a SIMD's 512 registers on the side stream, and waited for one of its
// workgroups to end: the chain column sums -> finalize -> apply of a 3.3 k-row map took 44 us beside it against 20.5 us with 4
// (17.5 -> 15.8 beside <3,3>, 9.9 -> 9.0 alone; profiles/r28_bn_finalize_in_apply_gate.txt).  The tree of the sums does not depend on it.
constexpr int FIN_COLS = 4, FIN_PARTS = 64;      // 64 slices: 8 dependent partial reads per thread at 512 row blocks (16 slices: 32 reads, 7.5 us per launch)

constexpr int FIN_ITERS = CR_MAX_BLOCKS / FIN_PARTS;     // partial blocks per thread (8)

__device__ inline void finalize_sums(const double* __restrict__ partial, int n_rb, int c, double& s1, double& s2,
                                     int& col) {
    __shared__ double red[2][FIN_PARTS][FIN_COLS];
    const int cl = threadIdx.x & (FIN_COLS - 1), part = threadIdx.x / FIN_COLS;
    col = blockIdx.x * FIN_COLS + cl;
    // all 2 x FIN_ITERS loads are issued before the first add (clamped addresses, masked afterwards): the kernel is
    // one memory round trip long instead of FIN_ITERS dependent ones (5 us -> 3 us per launch, 96 launches a step)
    double va[FIN_ITERS], vb[FIN_ITERS];
    const int cc = col < c ? col : 0;
#pragma unroll
    for (int i = 0; i < FIN_ITERS; ++i) {
        const int blk = part + FIN_PARTS * i;
        const int bc = blk < n_rb ? blk : 0;
        va[i] = partial[(int64_t(bc) * 2 + 0) * c + cc];
        vb[i] = partial[(int64_t(bc) * 2 + 1) * c + cc];
    }
    double a = 0, b = 0;
#pragma unroll
    for (int i = 0; i < FIN_ITERS; ++i) {
        const bool on = col < c && part + FIN_PARTS * i < n_rb;
        a += on ? va[i] : 0.0;
        b += on ? vb[i] : 0.0;
    }
    red[0][part][cl] = a;
    red[1][part][cl] = b;
    __syncthreads();
    // two levels, fixed order: slices 8 g .. 8 g + 7 by thread (g, cl), then the eight group sums by thread (0, cl)
    // (a single thread adding 64 slices is a chain of 128 dependent LDS reads + fp64 adds: 3 of the kernel's 5 us)
    double t1 = 0, t2 = 0;
    if (part < 8) {
#pragma unroll
        for (int q = 0; q < 8; ++q) { t1 += red[0][part * 8 + q][cl]; t2 += red[1][part * 8 + q][cl]; }
    }
    __syncthreads();
    if (part < 8) {
        red[0][part][cl] = t1;
        red[1][part][cl] = t2;
    }
    __syncthreads();
    s1 = 0; s2 = 0;
    if (part == 0) {
#pragma unroll
        for (int q = 0; q < 8; ++q) { s1 += red[0][q][cl]; s2 += red[1][q][cl]; }
    }
}

__global__ __launch_bounds__(FIN_COLS * FIN_PARTS) void bn_stats_finalize_kernel(
    const double* __restrict__ partial, int n_rb, int64_t n, int c, float* __restrict__ mean, float* __restrict__ var,
    float* __restrict__ running_mean, float* __restrict__ running_var, float momentum) {
    double s1, s2;
    int j;
    finalize_sums(partial, n_rb, c, s1, s2, j);
    if (threadIdx.x >= FIN_COLS || j >= c) return;
    const double m = s1 / double(n);
    double v = s2 / double(n) - m * m;
    if (v < 0) v = 0;
    mean[j] = float(m);
    var[j] = float(v);
    if (running_mean) running_mean[j] = (1.f - momentum) * running_mean[j] + momentum * float(m);
    if (running_var) {
        const double unb = n > 1 ? v * double(n) / double(n - 1) : v;
        running_var[j] = (1.f - momentum) * running_var[j] + momentum * float(unb);
    }
}

__global__ __launch_bounds__(FIN_COLS * FIN_PARTS) void bn_bwd_finalize_kernel(const double* __restrict__ partial,
                                                                              int n_rb, int c,
                                                                              float* __restrict__ sum_g,
                                                                              float* __restrict__ sum_gx) {
    double s1, s2;
    int j;
    finalize_sums(partial, n_rb, c, s1, s2, j);
    if (threadIdx.x >= FIN_COLS || j >= c) return;
    sum_g[j] = float(s1);
    sum_gx[j] = float(s2);
}

// The finalize step INSIDE a backward apply pass (small maps).  Up to FOLD_MAX_RB row blocks of column sums every apply workgroup
// forms the column totals it needs from the partials itself, instead of waiting for a launch of bn_bwd_finalize_kernel that moves a
// few kilobytes (48 launches a step).  What a workgroup reads is n_rb x 16 bytes per column it covers, so these
// launches walk the matrix in COLUMN GROUPS (GroupWalk below: a workgroup owns FOLD_COLS = 32 columns -- one 128-byte line per row --
// and 32 row lanes): at most 64 x 32 x 16 bytes = 32 KB out of L2, in ONE round trip -- thread (group g, column j) issues the 16 loads
// of its eight row blocks before the first add.  A workgroup that covered all c columns (the walks of the larger maps) read 106 KB on
// the 3.3 k-row x 128 level in 3.5 dependent rounds and lost 1 us against the separate launch, 13 us at 4096 x 256
// (profiles/r28_bn_finalize_in_apply_gate.txt).
// The price is read amplification, and it is why FOLD_MAX_RB stays where the plan of the column sums puts a 4096-row map: a workgroup
// moves a 32 x 32 tile (4 KB each of x, g, gx) and reads up to 32 KB of partials for it -- at 4096 x 256, 1024 workgroups x 32 KB =
// 32 MB out of L2 for a 4 MB matrix.  It measured 2.3 us faster there than the finalize launch; the ratio grows with n_rb.
// EXACTLY finalize_sums' tree, so every bit stays: slice `part` there holds block `part` (n_rb <= 64: one block per slice, 0 + v),
// eight slices are added in order from 0, then the eight group sums in order from 0.  What is left out are adds of +0.0 to a sum that
// started at +0.0 and so is never -0.0: identities.  The two totals of a column are left as floats in LDS, where the apply walk takes
// them as it took them from global memory; the workgroups of the first row chunk also write gbeta and ggamma, as
// bn_bwd_finalize_kernel does.
constexpr int FOLD_MAX_RB = 64, FOLD_COLS = 32, FOLD_ROWS = 256 / (FOLD_COLS / 4);
static_assert(FOLD_MAX_RB <= FIN_PARTS && FOLD_MAX_RB == 8 * (256 / FOLD_COLS), "one partial block per slice of finalize_sums, one (group, column) per thread");

// -> the totals in LDS: [2][FOLD_COLS], (sum g, sum g * xhat) of columns blockIdx.y * FOLD_COLS + j
__device__ __forceinline__ const float* fold_sums(const double* __restrict__ partial, int n_rb, int c, float* __restrict__ sum_g,
                                                  float* __restrict__ sum_gx) {
    __shared__ double grp[2][FOLD_MAX_RB / 8][FOLD_COLS];
    __shared__ __attribute__((aligned(16))) float tot[2][FOLD_COLS];
    const int ng = (n_rb + 7) >> 3;
    {
        const int g = threadIdx.x / FOLD_COLS, j = threadIdx.x % FOLD_COLS, col = blockIdx.y * FOLD_COLS + j;
        if (g < ng && col < c) {
            double va[8], vb[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int blk = g * 8 + q, bc = blk < n_rb ? blk : 0;
                va[q] = partial[(int64_t(bc) * 2 + 0) * c + col];
                vb[q] = partial[(int64_t(bc) * 2 + 1) * c + col];
            }
            double a = 0, b = 0;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const bool on = g * 8 + q < n_rb;
                a += on ? va[q] : 0.0;
                b += on ? vb[q] : 0.0;
            }
            grp[0][g][j] = a;
            grp[1][g][j] = b;
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * FOLD_COLS) {
        const int which = threadIdx.x / FOLD_COLS, j = threadIdx.x % FOLD_COLS, col = blockIdx.y * FOLD_COLS + j;
        if (col < c) {
            double t = 0;
            for (int g = 0; g < ng; ++g) t += grp[which][g][j];
            tot[which][j] = float(t);
            if (blockIdx.x == 0) (which ? sum_gx : sum_g)[col] = float(t);
        }
    }
    __syncthreads();
    return &tot[0][0];
}

// The apply passes (forward, backward, backward reading gres) are each written ONCE, over one of two walks through the quads of an
// [n, c] matrix, c4 = c / 4 quads a row.  Per-element expressions: epilogue.h.  Every element is read and then written by the same
// thread (in place is fine).
//   KEEP   the thread keeps its columns: the launch plan (plan_apply) makes the grid's stride a multiple of c4, so a thread's quads
//          all lie in one column quad, `stride / c4` rows apart.  Column and first row come from one 32-bit division, the column
//          constants (four 1 / sqrt among them) are taken once, and the walk advances offsets.  Per quad that leaves the loads that
//          carry new data and the per-element arithmetic: 35 VALU instructions and 2 loads on a forward pass.
//   flat   a grid-stride walk; column and constants are taken again for every quad (241 VALU instructions, 9 transcendental, 16 v_div_*,
//          and 6 loads: profiles/r24_bn_one_definition_resource_usage.txt).  Runs where no grid keeps a thread on its columns
//          (plan_apply: wide odd c4) and by osn_bn_set_flat_kernels(1).
template <bool KEEP>
struct QuadWalk {
    int64_t e, stride, row_, rstep;                          // quad index and its step; (KEEP) row and its step
    int col_;
    __device__ QuadWalk(int c4) {
        if constexpr (KEEP) {
            const unsigned e0 = blockIdx.x * 256u + threadIdx.x, s = gridDim.x * 256u;        // s % c4 == 0
            const unsigned row0 = e0 / unsigned(c4);
            col_ = int(e0 - row0 * unsigned(c4)) * 4;
            e = e0; stride = s; row_ = row0; rstep = s / unsigned(c4);
        } else {
            e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
            stride = int64_t(gridDim.x) * blockDim.x;
        }
    }
    __device__ int col(int c4) const { return KEEP ? col_ : int(e % c4) * 4; }
    __device__ int64_t row(int c4) const { return KEEP ? row_ : e / c4; }
    __device__ int64_t off() const { return e * 4; }         // element offset of the quad in a contiguous [n, c] matrix
    __device__ void next() {
        e += stride;
        if constexpr (KEEP) row_ += rstep;
    }
};

// The walk of the launches that finalize for themselves: workgroup (chunk of FOLD_ROWS rows, column group of FOLD_COLS), thread (row,
// column quad) -- ONE quad per thread (the grid covers every row: these maps have at most 4096), so the column constants are taken
// once, as in QuadWalk<true>.  A thread past the last row or the last column has nothing to walk.
struct GroupWalk {
    int64_t e, row_;
    int col_;
    __device__ GroupWalk(int c4) {
        col_ = blockIdx.y * FOLD_COLS + int(threadIdx.x % (FOLD_COLS / 4)) * 4;
        row_ = int64_t(blockIdx.x) * FOLD_ROWS + threadIdx.x / (FOLD_COLS / 4);
        e = col_ < c4 * 4 ? row_ * c4 + (col_ >> 2) : INT64_MAX;
    }
    __device__ int col(int) const { return col_; }
    __device__ int64_t row(int) const { return row_; }
    __device__ int64_t off() const { return e * 4; }
    __device__ void next() { e = INT64_MAX; }
};

template <bool KEEP>
__device__ __forceinline__ void bn_apply_body(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ var,
                                              const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                              const float* __restrict__ residual, int relu, float* __restrict__ y,
                                              float* __restrict__ y2, int64_t ld2, int64_t total4, int c4) {
    QuadWalk<KEEP> w(c4);
    if (w.e >= total4) return;
    EpiCols k;
    if (KEEP) k = epi_cols(mean, var, gamma, beta, eps, w.col(c4));
    for (; w.e < total4; w.next()) {
        const int col = w.col(c4);
        const int64_t o4 = w.off();
        if (!KEEP) k = epi_cols(mean, var, gamma, beta, eps, col);
        // (the residual is issued with x, ahead of the arithmetic: one round trip per quad)
        const float4 xv = ld4(x + o4), rv = residual ? ld4(residual + o4) : make_float4(0, 0, 0, 0);
        const float4 o = bn_fwd_quad(xv, k, residual != nullptr, [&] { return rv; }, relu);
        *reinterpret_cast<float4*>(y + o4) = o;
        // second store: the same rows as a column window of a wider matrix (ME.cat written in place by its producers)
        if (y2) *reinterpret_cast<float4*>(y2 + w.row(c4) * ld2 + col) = o;
    }
}

// LOAD_G: g was stored to gres by col_reduce_gres_kernel; y and the sources are not read and gres is not written.
// FOLD: the column totals come from fold_sums (above), not from a finalize launch: sum_g / sum_gx are then this launch's OUTPUTS
// (gbeta / ggamma) and `partial` holds the n_rb row blocks of the column sums; the walk is GroupWalk.  Batch statistics only.
template <bool KEEP, bool LOAD_G, bool FOLD = false>
__device__ __forceinline__ void bn_bwd_apply_body(const float* __restrict__ x, const float* __restrict__ y, const GySrc& gy,
                                                  const float* __restrict__ mean, const float* __restrict__ var,
                                                  const float* __restrict__ gamma, float eps, int relu, int training,
                                                  const float* __restrict__ sum_g, const float* __restrict__ sum_gx, float inv_n,
                                                  float* __restrict__ gx, float* __restrict__ gres, int64_t total4, int c4,
                                                  const float* __restrict__ beta, const double* __restrict__ partial = nullptr,
                                                  int n_rb = 0) {
    static_assert(!FOLD || KEEP, "a launch that finalizes for itself keeps its columns");
    const bool from_x = !LOAD_G && relu && !y;               // ReLU mask recomputed from x: one tensor less to read
    const float *sg = sum_g, *sx = sum_gx;                   // the two column totals as the walk reads them, and the index of column 0 in them
    int sum_col0 = 0;
    if constexpr (FOLD) {
        sg = fold_sums(partial, n_rb, c4 * 4, const_cast<float*>(sum_g), const_cast<float*>(sum_gx));
        sx = sg + FOLD_COLS;
        sum_col0 = blockIdx.y * FOLD_COLS;
    }
    std::conditional_t<FOLD, GroupWalk, QuadWalk<KEEP>> w(c4);
    if (w.e >= total4) return;
    BnBwdCols k;
    if (KEEP) k = bn_bwd_cols(mean, var, gamma, beta, sg, sx, eps, training, from_x, w.col(c4), w.col(c4) - sum_col0);
    for (; w.e < total4; w.next()) {
        const int col = w.col(c4);
        const int64_t o4 = w.off();
        if (!KEEP) k = bn_bwd_cols(mean, var, gamma, beta, sg, sx, eps, training, from_x, col, col);
        // every load of the quad first (x, the sources or gres, y), then the arithmetic: one round trip per quad
        float4 xv = make_float4(0, 0, 0, 0), yv, gs[BN_MAX_SRC];
        if (training || from_x) xv = ld4(x + o4);
        if (LOAD_G) {
            gs[0] = ld4(gres + o4);                          // (already summed and masked)
        } else {
            gy_load(gs, gy, w.row(c4), col);
            if (relu && !from_x) yv = ld4(y + o4);
        }
        const float4 g = bn_masked_grad(gs, LOAD_G ? 1 : gy.n, xv, yv, k.c, !LOAD_G && relu, from_x);
        if (!LOAD_G && gres) *reinterpret_cast<float4*>(gres + o4) = g;
        *reinterpret_cast<float4*>(gx + o4) = bn_bwd_quad(g, xv, k, inv_n, training);
    }
}

#define OSN_BN_APPLY_PARAMS                                                                                                    \
    const float *__restrict__ x, const float *__restrict__ mean, const float *__restrict__ var, const float *__restrict__ gamma,  \
        const float *__restrict__ beta, float eps, const float *__restrict__ residual, int relu, float *__restrict__ y,          \
        float *__restrict__ y2, int64_t ld2, int64_t total4, int c4
#define OSN_BN_BWD_PARAMS                                                                                                      \
    const float *__restrict__ x, const float *__restrict__ y, const GySrc gy, const float *__restrict__ mean,                    \
        const float *__restrict__ var, const float *__restrict__ gamma, float eps, int relu, int training,                       \
        const float *__restrict__ sum_g, const float *__restrict__ sum_gx, float inv_n, float *__restrict__ gx,                  \
        float *__restrict__ gres, int64_t total4, int c4, const float *__restrict__ beta
#define OSN_BN_BWD_GRES_PARAMS                                                                                                 \
    const float *__restrict__ x, const float *__restrict__ mean, const float *__restrict__ var, const float *__restrict__ gamma,  \
        float eps, int training, const float *__restrict__ sum_g, const float *__restrict__ sum_gx, float inv_n,                 \
        float *__restrict__ gx, const float *__restrict__ gres, int64_t total4, int c4

__global__ __launch_bounds__(256) void bn_apply_kernel(OSN_BN_APPLY_PARAMS) {
    bn_apply_body<true>(x, mean, var, gamma, beta, eps, residual, relu, y, y2, ld2, total4, c4);
}
__global__ __launch_bounds__(256) void bn_apply_flat_kernel(OSN_BN_APPLY_PARAMS) {
    bn_apply_body<false>(x, mean, var, gamma, beta, eps, residual, relu, y, y2, ld2, total4, c4);
}
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(OSN_BN_BWD_PARAMS) {
    bn_bwd_apply_body<true, false>(x, y, gy, mean, var, gamma, eps, relu, training, sum_g, sum_gx, inv_n, gx, gres, total4, c4, beta);
}
__global__ __launch_bounds__(256) void bn_bwd_apply_flat_kernel(OSN_BN_BWD_PARAMS) {
    bn_bwd_apply_body<false, false>(x, y, gy, mean, var, gamma, eps, relu, training, sum_g, sum_gx, inv_n, gx, gres, total4, c4, beta);
}
__global__ __launch_bounds__(256) void bn_bwd_apply_gres_kernel(OSN_BN_BWD_GRES_PARAMS) {
    bn_bwd_apply_body<true, true>(x, nullptr, GySrc{}, mean, var, gamma, eps, 0, training, sum_g, sum_gx, inv_n, gx,
                                  const_cast<float*>(gres), total4, c4, nullptr);
}
__global__ __launch_bounds__(256) void bn_bwd_apply_gres_flat_kernel(OSN_BN_BWD_GRES_PARAMS) {
    bn_bwd_apply_body<false, true>(x, nullptr, GySrc{}, mean, var, gamma, eps, 0, training, sum_g, sum_gx, inv_n, gx,
                                   const_cast<float*>(gres), total4, c4, nullptr);
}

// The two kernels that keep their columns, with the finalize step inside (bn_bwd_apply_body<.., FOLD>): `fin` = the workgroup finalizes
// for itself.  Grid (row chunks, column groups of FOLD_COLS).
__global__ __launch_bounds__(256) void bn_bwd_apply_fin_kernel(
    const float* __restrict__ x, const float* __restrict__ y, const GySrc gy, const float* __restrict__ mean, const float* __restrict__ var,
    const float* __restrict__ gamma, float eps, int relu, float* __restrict__ gbeta, float* __restrict__ ggamma, float inv_n,
    float* __restrict__ gx, float* __restrict__ gres, int64_t total4, int c4, const float* __restrict__ beta,
    const double* __restrict__ partial, int n_rb) {
    bn_bwd_apply_body<true, false, true>(x, y, gy, mean, var, gamma, eps, relu, 1, gbeta, ggamma, inv_n, gx, gres, total4, c4, beta, partial, n_rb);
}
__global__ __launch_bounds__(256) void bn_bwd_apply_gres_fin_kernel(
    const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ var, const float* __restrict__ gamma, float eps,
    float* __restrict__ gbeta, float* __restrict__ ggamma, float inv_n, float* __restrict__ gx, const float* __restrict__ gres,
    int64_t total4, int c4, const double* __restrict__ partial, int n_rb) {
    bn_bwd_apply_body<true, true, true>(x, nullptr, GySrc{}, mean, var, gamma, eps, 0, 1, gbeta, ggamma, inv_n, gx, const_cast<float*>(gres),
                                        total4, c4, nullptr, partial, n_rb);
}

// ---------------------------------------------------------------------------------------------------------------
// Small maps (the deep U-Net levels: 700 - 3 000 rows): the three launches of a training-mode batch norm (column sums,
// finalize, apply) are each a few microseconds of launch latency around almost no work.  Up to SB_MAX_ROWS rows one
// workgroup of 1024 threads owns 8 columns, keeps its rows IN REGISTERS between the statistics and the apply pass (x is
// read once), and reduces with wave shuffles + one LDS round in a fixed order (deterministic).  Same formulas as the
// three-kernel path (fp64 sums, fp32 mean / var / apply).  Measured (profiles/r03_s3): 14.5 us per launch against
// ~15 us for the three launches it replaces -- a tie in GPU time, two launches (and their gaps) fewer.  The same design
// for the BACKWARD pass (x, y and up to three gradient sources per row in registers) was slower (24 us against 14 us)
// and is not kept.
constexpr int SB_THREADS = 1024, SB_RL = 512, SB_PER = 8, SB_COLS = 8;
constexpr int SB_MAX_ROWS = SB_RL * SB_PER;       // 4096

__device__ inline double sb_wave_sum(double v) {
    // lanes of one wave that share bit 0 (the column lane): xor-shuffle over the 32 row lanes
#pragma unroll
    for (int off = 2; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// sums[0..3] / sums[4..7] of this thread's 4 columns -> totals over the workgroup's rows, in every thread
__device__ inline void sb_block_sums(double (&s)[8], int tid, int cl) {
    __shared__ double red[SB_THREADS / 64][2][8];
    __shared__ double tot[2][8];
#pragma unroll
    for (int q = 0; q < 8; ++q) s[q] = sb_wave_sum(s[q]);
    const int lane = tid & 63, wave = tid >> 6;
    if ((lane >> 1) == 0) {
#pragma unroll
        for (int q = 0; q < 8; ++q) red[wave][cl][q] = s[q];
    }
    __syncthreads();
    if (tid < 16) {
        const int c2 = tid >> 3, q = tid & 7;
        double t = 0;
#pragma unroll
        for (int w = 0; w < SB_THREADS / 64; ++w) t += red[w][c2][q];
        tot[c2][q] = t;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) s[q] = tot[cl][q];
}

__global__ __launch_bounds__(SB_THREADS) void bn_small_fwd_kernel(const float* __restrict__ x, int n, int c,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  float eps, const float* __restrict__ residual, int relu,
                                                                  float momentum, float* __restrict__ mean_out,
                                                                  float* __restrict__ var_out, float* __restrict__ running_mean,
                                                                  float* __restrict__ running_var, float* __restrict__ y,
                                                                  float* __restrict__ y2, int64_t ld2) {
    const int tid = threadIdx.x, cl = tid & 1, rl = tid >> 1;
    const int col = blockIdx.x * SB_COLS + cl * 4;
    const bool con = col < c;
    const int cc = con ? col : 0;
    float4 v[SB_PER];
    double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < SB_PER; ++j) {
        const int r = rl + SB_RL * j;
        const bool ok = con && r < n;
        v[j] = ld4(x + int64_t(ok ? r : 0) * c + cc);
        if (ok) {
            s[0] += v[j].x; s[1] += v[j].y; s[2] += v[j].z; s[3] += v[j].w;
            s[4] += double(v[j].x) * v[j].x; s[5] += double(v[j].y) * v[j].y;
            s[6] += double(v[j].z) * v[j].z; s[7] += double(v[j].w) * v[j].w;
        }
    }
    sb_block_sums(s, tid, cl);
    float mu[4], vr[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double m = s[q] / double(n);
        double var = s[4 + q] / double(n) - m * m;
        if (var < 0) var = 0;
        mu[q] = float(m);
        vr[q] = float(var);
        if (rl == 0 && con) {
            mean_out[col + q] = mu[q];
            var_out[col + q] = vr[q];
            if (running_mean) running_mean[col + q] = (1.f - momentum) * running_mean[col + q] + momentum * mu[q];
            if (running_var) {
                const double unb = n > 1 ? var * double(n) / double(n - 1) : var;
                running_var[col + q] = (1.f - momentum) * running_var[col + q] + momentum * float(unb);
            }
        }
    }
    if (!con) return;
    const EpiCols k{make_float4(mu[0], mu[1], mu[2], mu[3]),
                    make_float4(bn_is(vr[0], eps), bn_is(vr[1], eps), bn_is(vr[2], eps), bn_is(vr[3], eps)), ld4(gamma + col), ld4(beta + col)};
#pragma unroll
    for (int j = 0; j < SB_PER; ++j) {
        const int r = rl + SB_RL * j;
        if (r >= n) continue;
        const float4 o = bn_fwd_quad(v[j], k, residual != nullptr, [&] { return ld4(residual + int64_t(r) * c + col); }, relu);
        *reinterpret_cast<float4*>(y + int64_t(r) * c + col) = o;
        if (y2) *reinterpret_cast<float4*>(y2 + int64_t(r) * ld2 + col) = o;
    }
}

// [a, a + na) and [b, b + nb) floats share an address
static bool ranges_overlap(const float* a, size_t na, const float* b, size_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + nb * sizeof(float) && b0 < a0 + na * sizeof(float);
}

static int ew_grid(int64_t total4) {
    int64_t g = cdiv(total4, 256);
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return int(g);
}

// The apply kernels' launch plan, stated once: the smallest grid >= ew_grid(total4) whose stride (grid x 256 quads) is a multiple of
// c4 -- a multiple of c4 / gcd(c4, 256) -- at most EW_SLACK workgroups above it (workgroups past the last quad leave at once, but a
// wide odd c4 would ask for up to c4 - 1 of them).  keep = false: no such grid, the flat kernels run on ew_grid(total4).
constexpr int EW_SLACK = 127;
struct ApplyPlan {
    int grid;
    bool keep;
};

static ApplyPlan plan_apply(int64_t total4, int c4) {
    const int g = ew_grid(total4);
    int a = c4, b = 256;
    while (b) { const int t = a % b; a = b; b = t; }
    const int64_t m = c4 / a;
    const int64_t up = cdiv(int64_t(g), m) * m;
    if (up - g <= EW_SLACK) return ApplyPlan{int(up), true};
    return ApplyPlan{g, false};
}

// osn_bn_set_flat_kernels: the kernels of the earlier rounds (flat apply walks, one row in flight in the column sums)
static std::atomic<int> g_flat_kernels{0};

// osn_bn_set_separate_finalize: bn_bwd_finalize_kernel as a launch of its own on every map (tests, A/B)
static std::atomic<int> g_separate_finalize{0};

#ifndef OSN_BN_KEEP_COLUMNS
#define OSN_BN_KEEP_COLUMNS 1                                // 0: an A/B build whose apply passes are always the flat kernels
#endif

static ApplyPlan launch_plan_apply(int64_t total4, int c4) {
    if (!OSN_BN_KEEP_COLUMNS || g_flat_kernels.load(std::memory_order_relaxed)) return ApplyPlan{ew_grid(total4), false};
    return plan_apply(total4, c4);
}

// The pointers of a forward pass.  quad_stats: mean and var are read as quads (the apply kernels; the one-launch kernel writes them
// element by element).
static int check_fwd_args(const char* who, const float* x, const float* mean, const float* var, bool quad_stats, const float* gamma,
                          const float* beta, const float* residual, const float* y, const float* y2, int64_t ld2, int c) {
    OSN_REQUIRE(x && mean && var && gamma && beta && y, OSN_E_ARG, "%s: null pointer", who);
    OSN_REQUIRE(aligned16(x) && aligned16(y) && (!quad_stats || (aligned16(mean) && aligned16(var))) && aligned16(gamma) &&
                    aligned16(beta) && (!residual || aligned16(residual)),
                OSN_E_ARG, "%s: pointers must be 16-byte aligned", who);
    OSN_REQUIRE(!y2 || (aligned16(y2) && ld2 >= c && (ld2 & 3) == 0), OSN_E_ARG,
                "%s: the second destination needs a 16-byte aligned pointer and a row stride >= c, %% 4 == 0", who);
    return OSN_OK;
}

}  // namespace osn

using namespace osn;

extern "C" int osn_bn_set_flat_kernels(int on) { return g_flat_kernels.exchange(on ? 1 : 0); }

extern "C" int osn_bn_set_separate_finalize(int on) { return g_separate_finalize.exchange(on ? 1 : 0); }

extern "C" int osn_bn_apply_plan(int64_t total4, int c4, int* grid, int* flat) {
    OSN_REQUIRE(total4 >= 0 && c4 >= 1 && grid && flat, OSN_E_ARG, "osn_bn_apply_plan: need total4 >= 0, c4 >= 1 and two outputs");
    const ApplyPlan p = plan_apply(total4, c4);
    *grid = p.grid;
    *flat = p.keep ? 0 : 1;
    return OSN_OK;
}

extern "C" size_t osn_bn_ws_bytes(int64_t n, int c) {
    (void)n;
    return size_t(CR_MAX_BLOCKS) * 2 * size_t(c) * 8 + 256;
}

extern "C" int osn_bn_stats(const float* x, int64_t n, int c, float* mean, float* var, float* running_mean,
                            float* running_var, float momentum, void* ws, size_t ws_bytes, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(n >= 1 && c >= 4 && (c & 3) == 0, OSN_E_ARG, "osn_bn_stats: need n >= 1 and c %% 4 == 0 (n=%lld c=%d)", (long long)n, c);
    OSN_REQUIRE(x && mean && var && aligned16(x), OSN_E_ARG, "osn_bn_stats: null or unaligned pointer");
    ColReducePlan p = plan_colreduce(n, c);
    const size_t need = size_t(p.n_rb) * 2 * size_t(c) * 8;
    OSN_REQUIRE(ws && ws_bytes >= need, OSN_E_WS, "osn_bn_stats: workspace %zu < %zu", ws_bytes, need);
    double* partial = static_cast<double*>(ws);
    const auto kern = g_flat_kernels.load(std::memory_order_relaxed) ? col_reduce_1row_kernel<0> : col_reduce_kernel<0>;
    hipLaunchKernelGGL(kern, dim3(p.n_rb, p.n_cg), dim3(256), 0, st, x, (const float*)nullptr,
                       GySrc{}, (const float*)nullptr, (const float*)nullptr, 0.f, 0, n, c,
                       p.rows_per_block, partial, (const float*)nullptr, (const float*)nullptr);
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(cdiv(c, FIN_COLS)), dim3(FIN_COLS * FIN_PARTS), 0, st, partial, p.n_rb, n, c, mean, var,
                       running_mean, running_var, momentum);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_bn_apply(const float* x, const float* mean, const float* var, const float* gamma, const float* beta,
                            float eps, const float* residual, int relu, float* y, float* y2, int64_t ld2, int64_t n, int c,
                            osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(n >= 0 && c >= 4 && (c & 3) == 0, OSN_E_ARG, "osn_bn_apply: need c %% 4 == 0 (c=%d)", c);
    if (n == 0) return OSN_OK;
    if (int rc = check_fwd_args("osn_bn_apply", x, mean, var, true, gamma, beta, residual, y, y2, ld2, c)) return rc;
    const int64_t total4 = n * (c / 4);
    const ApplyPlan ap = launch_plan_apply(total4, c / 4);
    hipLaunchKernelGGL(ap.keep ? bn_apply_kernel : bn_apply_flat_kernel, dim3(ap.grid), dim3(256), 0, st, x, mean, var, gamma, beta, eps,
                       residual, relu, y, y2, ld2, total4, c / 4);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

// Training-mode forward in ONE call: statistics (+ running buffers) and the fused normalise (+ residual) (+ ReLU) pass
// (+ the second destination of osn_bn_apply).  Up to SB_MAX_ROWS rows: ONE launch (bn_small_fwd_kernel); above: the
// kernels of osn_bn_stats + osn_bn_apply.
extern "C" int osn_bn_forward_train(const float* x, int64_t n, int c, const float* gamma, const float* beta, float eps,
                                    const float* residual, int relu, float momentum, float* mean, float* var,
                                    float* running_mean, float* running_var, float* y, float* y2, int64_t ld2, void* ws,
                                    size_t ws_bytes, osn_stream_t stream) {
    if (n >= 1 && n <= SB_MAX_ROWS && c >= 4 && (c & 3) == 0) {
        hipStream_t st = static_cast<hipStream_t>(stream);
        if (int rc = check_fwd_args("osn_bn_forward_train", x, mean, var, false, gamma, beta, residual, y, y2, ld2, c)) return rc;
        hipLaunchKernelGGL(bn_small_fwd_kernel, dim3(unsigned(cdiv(c, SB_COLS))), dim3(SB_THREADS), 0, st, x, int(n), c, gamma,
                           beta, eps, residual, relu, momentum, mean, var, running_mean, running_var, y, y2, ld2);
        OSN_LAUNCH_CHECK();
        return OSN_OK;
    }
    int rc = osn_bn_stats(x, n, c, mean, var, running_mean, running_var, momentum, ws, ws_bytes, stream);
    if (rc) return rc;
    return osn_bn_apply(x, mean, var, gamma, beta, eps, residual, relu, y, y2, ld2, n, c, stream);
}

extern "C" int osn_bn_backward(const float* x, const float* y, const float* const* gy, const int64_t* gy_ld, int n_gy,
                               const float* mean, const float* var, const float* gamma, const float* beta, float eps, int relu,
                               int training, float* gx, float* gres, float* ggamma, float* gbeta, int64_t n, int c,
                               void* ws, size_t ws_bytes, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(n >= 1 && c >= 4 && (c & 3) == 0, OSN_E_ARG, "osn_bn_backward: need n >= 1 and c %% 4 == 0");
    OSN_REQUIRE(gy && gy_ld && n_gy >= 1 && n_gy <= BN_MAX_SRC, OSN_E_ARG,
                "osn_bn_backward: %d gradient sources (1 .. %d are supported)", n_gy, BN_MAX_SRC);
    // y == null with relu: the mask is recomputed from x (the forward expression, bit for bit) -- needs beta, and a batch
    // norm WITHOUT a residual (with one, y = relu(bn(x) + residual) cannot be rebuilt from x alone)
    OSN_REQUIRE(x && mean && var && gamma && gx && ggamma && gbeta && (!relu || y || beta), OSN_E_ARG,
                "osn_bn_backward: null pointer (relu needs y, or beta to recompute the mask from x)");
    OSN_REQUIRE(!(relu && !y) || !gres, OSN_E_ARG, "osn_bn_backward: the ReLU mask can be recomputed from x only without a residual");
    OSN_REQUIRE(!beta || aligned16(beta), OSN_E_ARG, "osn_bn_backward: beta must be 16-byte aligned");
    OSN_REQUIRE(aligned16(x) && aligned16(gx) && aligned16(mean) && aligned16(var) && aligned16(gamma) &&
                    aligned16(ggamma) && aligned16(gbeta) && (!y || aligned16(y)) && (!gres || aligned16(gres)),
                OSN_E_ARG, "osn_bn_backward: pointers must be 16-byte aligned");
    GySrc src{};
    src.n = n_gy;
    for (int i = 0; i < BN_MAX_SRC; ++i) {
        const int j = i < n_gy ? i : 0;                  // unused slots repeat source 0 (never read)
        OSN_REQUIRE(gy[j] && aligned16(gy[j]) && gy_ld[j] >= c && (gy_ld[j] & 3) == 0, OSN_E_ARG,
                    "osn_bn_backward: gradient source %d needs a 16-byte aligned pointer and a row stride >= c, %% 4 == 0", j);
        src.p[i] = gy[j];
        src.ld[i] = gy_ld[j];
    }
    ColReducePlan p = plan_colreduce(n, c);
    const size_t need = size_t(p.n_rb) * 2 * size_t(c) * 8;
    OSN_REQUIRE(ws && ws_bytes >= need, OSN_E_WS, "osn_bn_backward: workspace %zu < %zu", ws_bytes, need);
    double* partial = static_cast<double*>(ws);
    // A residual's gradient is stored by the reduction and read back by the apply pass -- unless gres overlaps x, y, gx or a
    // source: the reduction would then overwrite rows another workgroup has yet to read, so the apply pass forms g itself as before.
    const size_t span = size_t(n) * size_t(c);
    bool via_gres = gres != nullptr && !ranges_overlap(gres, span, x, span) && !(y && ranges_overlap(gres, span, y, span)) &&
                    !ranges_overlap(gres, span, gx, span);
    for (int i = 0; via_gres && i < n_gy; ++i)
        via_gres = !ranges_overlap(gres, span, src.p[i], size_t(n - 1) * size_t(src.ld[i]) + size_t(c));
    const dim3 rgrid(p.n_rb, p.n_cg);
    const bool one_row = g_flat_kernels.load(std::memory_order_relaxed) != 0;
    // the kernel of the column sums by its ReLU mask: none, from x (no y given) or from y
    const int mask = !relu ? CR_MASK_NONE : (y ? CR_MASK_Y : CR_MASK_X);
    if (via_gres) {
        const auto kern = one_row ? col_reduce_gres_1row_kernel : col_reduce_gres_kernel;
        hipLaunchKernelGGL(kern, rgrid, dim3(256), 0, st, x, y, src, mean, var, eps, relu, n, c, p.rows_per_block, partial, gres);
    } else {
        const auto kern = one_row ? col_reduce_1row_kernel<1>
                                  : (mask == CR_MASK_X ? col_reduce_kernel<1, CR_MASK_X>
                                                       : (mask == CR_MASK_Y ? col_reduce_kernel<1, CR_MASK_Y> : col_reduce_kernel<1, CR_MASK_NONE>));
        hipLaunchKernelGGL(kern, rgrid, dim3(256), 0, st, x, y, src, mean, var, eps, relu, n, c, p.rows_per_block, partial, gamma, beta);
    }
    const int64_t total4 = n * (c / 4);
    // ggamma = sum g*xhat, gbeta = sum g  (also the two column sums the apply pass needs): a launch of its own, or -- small maps, batch
    // statistics -- formed by every apply workgroup for its columns and written by those of the first row chunk (fold_sums)
    const bool fold = training && p.n_rb <= FOLD_MAX_RB && !one_row && !g_separate_finalize.load(std::memory_order_relaxed);
    if (fold) {
        const dim3 fgrid(unsigned(cdiv(n, FOLD_ROWS)), unsigned(cdiv(c, FOLD_COLS)));
        if (via_gres)
            hipLaunchKernelGGL(bn_bwd_apply_gres_fin_kernel, fgrid, dim3(256), 0, st, x, mean, var, gamma, eps, gbeta, ggamma, 1.f / float(n), gx,
                               (const float*)gres, total4, c / 4, (const double*)partial, p.n_rb);
        else
            hipLaunchKernelGGL(bn_bwd_apply_fin_kernel, fgrid, dim3(256), 0, st, x, y, src, mean, var, gamma, eps, relu, gbeta, ggamma,
                               1.f / float(n), gx, gres, total4, c / 4, beta, (const double*)partial, p.n_rb);
        OSN_LAUNCH_CHECK();
        return OSN_OK;
    }
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(cdiv(c, FIN_COLS)), dim3(FIN_COLS * FIN_PARTS), 0, st, partial, p.n_rb, c, gbeta, ggamma);
    const ApplyPlan ap = launch_plan_apply(total4, c / 4);
    if (via_gres)
        hipLaunchKernelGGL(ap.keep ? bn_bwd_apply_gres_kernel : bn_bwd_apply_gres_flat_kernel, dim3(ap.grid), dim3(256), 0, st, x, mean,
                           var, gamma, eps, training, gbeta, ggamma, 1.f / float(n), gx, (const float*)gres, total4, c / 4);
    else
        hipLaunchKernelGGL(ap.keep ? bn_bwd_apply_kernel : bn_bwd_apply_flat_kernel, dim3(ap.grid), dim3(256), 0, st, x, y, src, mean, var,
                           gamma, eps, relu, training, gbeta, ggamma, 1.f / float(n), gx, gres, total4, c / 4, beta);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}
