// Supervised segmentation head (the MinkowskiNet baseline): cross-entropy with ignore_index, argmax, confusion matrix and
// the test-repeat vote, forward and backward in one streaming pass each.
//
// Replaces run/train_mink.py:160,279-290,367-372 and util/util.py:132-145:
//     loss = nn.CrossEntropyLoss(ignore_index=255)(output, label)
//     output = output.detach().max(1)[1]
//     intersection, union, target = intersectionAndUnionGPU(output, label, classes, 255)     (three host copies + histc)
// util/metric.py:9-25 (the confusion matrix in numpy) and run/eval_mink.py:184-216 (votes summed on the host).
// The forward pass reads each row once and leaves per-workgroup loss partials (fp64, fixed order) for a one-workgroup
// second launch; the backward pass reads the row again and writes d loss / d logits once.  A row of c <= 8 G classes lives
// in a group of G lanes (lane g holds columns g, g + G, ...: one group-wide load is G consecutive floats of the row), G per
// c bucket: 1 (c <= 8), 2 (<= 16), 4 (<= 32), 8 (<= 64), 16 (<= 128), 32 (<= 256).
#include "common.h"

namespace osn {

constexpr int SEG_PER = 8;              // logits per lane
constexpr int SEG_THREADS = 256;
constexpr int SEG_MAX_WG = 512;         // workgroups of the forward / backward grid-stride loops (the loss partials)
constexpr int SEG_HIST_MAX_C = 90;      // confusion histogram in LDS while c * c int32 fit in 32 KB; wider: global int64 atomics

template <int G>
__device__ inline float group_sum(float v) {
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// torch.max(dim=1)[1]: NaN is the largest value; among equal values the lowest column wins
__device__ inline bool seg_better(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v > bv || (v == bv && i < bi);
}

// One row held by a group: the logits, the row maximum, its column and s1 = sum_{k != argmax} exp(x_k - max).
// logsumexp(x) - max = log1p(s1): the term of the argmax (exactly 1) is kept out of the sum, so a confident row keeps its
// small loss instead of rounding 1 + s1 to 1.
template <int G>
struct SegRow {
    float v[SEG_PER];
    float m, s1;
    int bi;

    __device__ inline void load(const float* __restrict__ x, int c, int g) {
        float bv = -INFINITY;
        bi = 0x7fffffff;
#pragma unroll
        for (int t = 0; t < SEG_PER; ++t) {
            const int k = g + G * t;
            v[t] = k < c ? x[k] : -INFINITY;
            if (k < c && seg_better(v[t], k, bv, bi)) { bv = v[t]; bi = k; }
        }
#pragma unroll
        for (int msk = G / 2; msk >= 1; msk >>= 1) {
            const float ov = __shfl_xor(bv, msk, 64);
            const int oi = __shfl_xor(bi, msk, 64);
            if (seg_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        m = bv;                               // NaN when the row holds one: every exp below is NaN then, as is torch's loss
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < SEG_PER; ++t) {
            const int k = g + G * t;
            if (k < c && k != bi) s += expf(v[t] - m);
        }
        s1 = group_sum<G>(s);
        // A maximum that is not finite (+inf; -inf: every logit is -inf; the lone NaN of c = 1) has no softmax: torch's row loss
        // and every element of the row's gradient are NaN.  Left alone, a +inf row has s1 = 0 (exp(-inf) elsewhere, the argmax
        // kept out): a finite gradient from an overflowed logit.  Rows with a finite maximum keep their bits.
        if (!(fabsf(m) < INFINITY)) s1 = __builtin_nanf("");
    }

    __device__ inline float at(int y, int g) const {      // x[y] (every lane of the group gets it)
        float r = 0.f;
#pragma unroll
        for (int t = 0; t < SEG_PER; ++t)
            if (g + G * t == y) r = v[t];
        return group_sum<G>(r);
    }
};

// rows of the grid-stride loop: row j of the labels reads logits row (rows ? rows[j] : j)
template <int G>
__global__ __launch_bounds__(SEG_THREADS) void seg_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ rows,
                                                              const int64_t* __restrict__ labels, int64_t n, int64_t n_lab, int c,
                                                              int64_t ignore, int64_t* __restrict__ pred,
                                                              unsigned long long* __restrict__ conf, int hist,
                                                              double* __restrict__ part, int64_t* __restrict__ part_n,
                                                              int32_t* __restrict__ err) {
    extern __shared__ unsigned int sh_hist[];          // [c * c] when hist
    __shared__ double red[SEG_THREADS];
    __shared__ int64_t red_n[SEG_THREADS];
    constexpr int RPI = SEG_THREADS / G;               // rows per workgroup and iteration
    const int tid = threadIdx.x, g = tid & (G - 1);
    if (hist) {
        for (int i = tid; i < c * c; i += SEG_THREADS) sh_hist[i] = 0;
        __syncthreads();
    }
    double acc = 0.0;
    int64_t cnt = 0;
    int e = 0;
    for (int64_t j0 = int64_t(blockIdx.x) * RPI; j0 < n_lab; j0 += int64_t(gridDim.x) * RPI) {
        const int64_t j = j0 + tid / G;
        if (j >= n_lab) continue;                      // uniform over a group: the shuffles stay inside live groups
        int64_t r = rows ? rows[j] : j;
        const int64_t y = labels[j];
        bool lab = y != ignore;
        if (lab && (y < 0 || y >= c)) { e |= 1; lab = false; }
        if (r < 0 || r >= n) { e |= 2; r = 0; lab = false; }
        SegRow<G> row;
        row.load(logits + r * c, c, g);
        const float xy = row.at(lab ? int(y) : -1, g);
        if (g == 0) {
            if (pred) pred[j] = row.bi == 0x7fffffff ? 0 : row.bi;
            if (lab) {
                acc += double((row.m - xy) + log1pf(row.s1));    // (m - x[y]: exact by Sterbenz while m / 2 <= x[y], else one rounding)
                ++cnt;
                if (conf) {
                    const int cell = row.bi * c + int(y);
                    if (hist) atomicAdd(&sh_hist[cell], 1u);
                    else atomicAdd(&conf[cell], 1ull);
                }
            }
        }
    }
    if (e) atomicOr(err, e);
    red[tid] = acc;
    red_n[tid] = cnt;
    __syncthreads();
    for (int w = SEG_THREADS / 2; w >= 1; w >>= 1) {
        if (tid < w) { red[tid] += red[tid + w]; red_n[tid] += red_n[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) { part[blockIdx.x] = red[0]; part_n[blockIdx.x] = red_n[0]; }
    if (hist)                                           // (the tree above ended on a barrier: every LDS add is in)
        for (int i = tid; i < c * c; i += SEG_THREADS)
            if (sh_hist[i]) atomicAdd(&conf[i], (unsigned long long)sh_hist[i]);
}

// second level, one workgroup, fixed order: loss = sum / n_valid (NaN when nothing is labelled), n_valid kept for backward
__global__ __launch_bounds__(SEG_THREADS) void seg_mean_kernel(const double* __restrict__ part, const int64_t* __restrict__ part_n,
                                                               int nb, float* __restrict__ loss, int64_t* __restrict__ n_valid) {
    __shared__ double red[SEG_THREADS];
    __shared__ int64_t red_n[SEG_THREADS];
    const int tid = threadIdx.x;
    double s = 0.0;
    int64_t k = 0;
    for (int b = tid; b < nb; b += SEG_THREADS) { s += part[b]; k += part_n[b]; }
    red[tid] = s;
    red_n[tid] = k;
    __syncthreads();
    for (int w = SEG_THREADS / 2; w >= 1; w >>= 1) {
        if (tid < w) { red[tid] += red[tid + w]; red_n[tid] += red_n[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) {
        *n_valid = red_n[0];
        if (loss) *loss = red_n[0] > 0 ? float(red[0] / double(red_n[0])) : __builtin_nanf("");
    }
}

// glogits[i] = gloss (softmax(x_i) - onehot(y_i)) / n_valid on labelled rows, 0 on the others
template <int G>
__global__ __launch_bounds__(SEG_THREADS) void seg_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                              const float* __restrict__ gloss, const int64_t* __restrict__ n_valid,
                                                              int64_t n, int c, int64_t ignore, float* __restrict__ glogits) {
    constexpr int RPI = SEG_THREADS / G;
    const int tid = threadIdx.x, g = tid & (G - 1);
    const int64_t nv = *n_valid;
    const float sc = nv > 0 ? (gloss ? *gloss : 1.f) / float(nv) : 0.f;
    for (int64_t j0 = int64_t(blockIdx.x) * RPI; j0 < n; j0 += int64_t(gridDim.x) * RPI) {
        const int64_t j = j0 + tid / G;
        if (j >= n) continue;
        const int64_t y = labels[j];
        float* out = glogits + j * c;
        if (nv == 0 || y == ignore || y < 0 || y >= c) {
#pragma unroll
            for (int t = 0; t < SEG_PER; ++t)
                if (g + G * t < c) out[g + G * t] = 0.f;
            continue;
        }
        SegRow<G> row;
        row.load(logits + j * c, c, g);
        const float inv = 1.f / (1.f + row.s1);
#pragma unroll
        for (int t = 0; t < SEG_PER; ++t) {
            const int k = g + G * t;
            if (k >= c) continue;
            float p;
            if (k == row.bi) p = k == y ? -row.s1 * inv : inv;           // 1 / (1 + s1) - 1 without the cancellation
            else p = expf(row.v[t] - row.m) * inv - (k == y ? 1.f : 0.f);
            out[k] = sc * p;
        }
    }
}

// votes[p] += logits[rows ? rows[p] : p]   (a rows entry outside [0, n) adds nothing)
template <int G>
__global__ __launch_bounds__(SEG_THREADS) void seg_vote_kernel(const float* __restrict__ logits, const int64_t* __restrict__ rows,
                                                               int64_t n, int64_t n_pts, int c, float* __restrict__ votes) {
    constexpr int RPI = SEG_THREADS / G;
    const int64_t p = int64_t(blockIdx.x) * RPI + threadIdx.x / G;
    const int g = threadIdx.x & (G - 1);
    if (p >= n_pts) return;
    const int64_t r = rows ? rows[p] : p;
    if (r < 0 || r >= n) return;
    const float* x = logits + r * c;
    float* v = votes + p * c;
    for (int k = g; k < c; k += G) v[k] += x[k];
}

inline int seg_group(int c) {
    return c <= 8 ? 1 : c <= 16 ? 2 : c <= 32 ? 4 : c <= 64 ? 8 : c <= 128 ? 16 : 32;
}

inline int seg_grid(int64_t rows, int c) {
    const int64_t g = cdiv(rows, SEG_THREADS / seg_group(c));
    return int(g < 1 ? 1 : g > SEG_MAX_WG ? SEG_MAX_WG : g);
}

struct SegState {
    double* part;
    int64_t* part_n;
    int64_t* n_valid;
    int32_t* err;
};

inline SegState seg_state(void* p) {
    char* b = static_cast<char*>(p);
    SegState s;
    s.part = reinterpret_cast<double*>(b);
    s.part_n = reinterpret_cast<int64_t*>(b + SEG_MAX_WG * 8);
    s.n_valid = reinterpret_cast<int64_t*>(b + SEG_MAX_WG * 16);
    s.err = reinterpret_cast<int32_t*>(b + SEG_MAX_WG * 16 + 8);
    return s;
}

}  // namespace osn

using namespace osn;

#define OSN_SEG_DISPATCH(G_, KERNEL, GRID, SMEM, ...)                                                               \
    switch (G_) {                                                                                                   \
        case 1: hipLaunchKernelGGL(KERNEL<1>, dim3(GRID), dim3(SEG_THREADS), SMEM, __VA_ARGS__); break;            \
        case 2: hipLaunchKernelGGL(KERNEL<2>, dim3(GRID), dim3(SEG_THREADS), SMEM, __VA_ARGS__); break;            \
        case 4: hipLaunchKernelGGL(KERNEL<4>, dim3(GRID), dim3(SEG_THREADS), SMEM, __VA_ARGS__); break;            \
        case 8: hipLaunchKernelGGL(KERNEL<8>, dim3(GRID), dim3(SEG_THREADS), SMEM, __VA_ARGS__); break;            \
        case 16: hipLaunchKernelGGL(KERNEL<16>, dim3(GRID), dim3(SEG_THREADS), SMEM, __VA_ARGS__); break;          \
        default: hipLaunchKernelGGL(KERNEL<32>, dim3(GRID), dim3(SEG_THREADS), SMEM, __VA_ARGS__); break;          \
    }

// state: loss partials double [512] | their row counts int64 [512] | n_valid int64 | error bits int32
extern "C" size_t osn_seg_loss_state_bytes(int64_t n_lab, int c) {
    (void)n_lab; (void)c;
    return SEG_MAX_WG * 16 + 256;
}

extern "C" int osn_seg_loss_fwd(const float* logits, const int64_t* rows, const int64_t* labels, int64_t n, int64_t n_lab, int c,
                                int64_t ignore_index, float* loss, int64_t* pred, int64_t* confusion, void* state,
                                size_t state_bytes, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(n >= 1 && n_lab >= 0 && n_lab <= (int64_t(1) << 31) && c >= 1 && c <= 256 && (rows || n_lab == n), OSN_E_ARG,
                "osn_seg_loss_fwd: n=%lld n_lab=%lld c=%d (needs n >= 1, 1 <= c <= 256, n_lab == n without rows)",
                (long long)n, (long long)n_lab, c);
    OSN_REQUIRE(logits && labels && state && state_bytes >= osn_seg_loss_state_bytes(n_lab, c), OSN_E_ARG,
                "osn_seg_loss_fwd: null pointer or state buffer too small");
    SegState s = seg_state(state);
    OSN_HIP(hipMemsetAsync(s.err, 0, 4, st));
    const int G = seg_group(c);
    const int nb = seg_grid(n_lab, c);
    const int hist = confusion && c <= SEG_HIST_MAX_C;
    const size_t smem = hist ? size_t(c) * c * 4 : 0;
    unsigned long long* conf = reinterpret_cast<unsigned long long*>(confusion);
    OSN_SEG_DISPATCH(G, seg_fwd_kernel, nb, smem, st, logits, rows, labels, n, n_lab, c, ignore_index, pred, conf, hist, s.part,
                     s.part_n, s.err);
    hipLaunchKernelGGL(seg_mean_kernel, dim3(1), dim3(SEG_THREADS), 0, st, s.part, s.part_n, nb, loss, s.n_valid);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_seg_loss_bwd(const float* logits, const int64_t* labels, const float* gloss, int64_t n, int c, int64_t ignore_index,
                                float* glogits, const void* state, size_t state_bytes, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(n >= 1 && n <= (int64_t(1) << 31) && c >= 1 && c <= 256, OSN_E_ARG, "osn_seg_loss_bwd: n=%lld c=%d", (long long)n, c);
    OSN_REQUIRE(logits && labels && glogits && state && state_bytes >= osn_seg_loss_state_bytes(n, c), OSN_E_ARG,
                "osn_seg_loss_bwd: null pointer or state buffer too small");
    SegState s = seg_state(const_cast<void*>(state));
    OSN_SEG_DISPATCH(seg_group(c), seg_bwd_kernel, seg_grid(n, c), 0, st, logits, labels, gloss, s.n_valid, n, c, ignore_index,
                     glogits);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

// 0 = fine; bit 0: a label outside [0, c) that is not ignore_index; bit 1: a rows entry outside [0, n)  (synchronises)
extern "C" int osn_seg_loss_check(const void* state, int64_t n, int64_t n_lab, int c, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(state, OSN_E_ARG, "osn_seg_loss_check: null state");
    SegState s = seg_state(const_cast<void*>(state));
    int32_t host = 0;
    OSN_HIP(hipMemcpyAsync(&host, s.err, 4, hipMemcpyDeviceToHost, st));
    OSN_HIP(hipStreamSynchronize(st));
    OSN_REQUIRE(host == 0, OSN_E_ARG, "osn_seg_loss: %s (n=%lld, n_lab=%lld, c=%d)",
                (host & 1) ? "a label is outside [0, c) and is not ignore_index" : "a rows entry is outside [0, n)", (long long)n,
                (long long)n_lab, c);
    return OSN_OK;
}

extern "C" int osn_seg_vote(const float* logits, const int64_t* rows, int64_t n, int64_t n_pts, int c, float* votes,
                            osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(n >= 1 && n_pts >= 0 && c >= 1 && c <= 256 && (rows || n_pts == n), OSN_E_ARG,
                "osn_seg_vote: n=%lld n_pts=%lld c=%d", (long long)n, (long long)n_pts, c);
    if (n_pts == 0) return OSN_OK;
    OSN_REQUIRE(logits && votes, OSN_E_ARG, "osn_seg_vote: null pointer");
    const int G = seg_group(c);
    const unsigned grid = unsigned(cdiv(n_pts, SEG_THREADS / G));
    OSN_SEG_DISPATCH(G, seg_vote_kernel, grid, 0, st, logits, rows, n, n_pts, c, votes);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}
