// Sparse pooling layers on gfx950 ([ME] MinkowskiSumPooling / AvgPooling / MaxPooling, MinkowskiGlobal{Sum,Avg,Max}Pooling,
// MinkowskiBroadcast{Addition,Multiplication}; the reference builds three of them in models/resnet_base.py:54,69,71).
//
//   local    y[o] = reduce over the present k of x[nbr[k, o]]     one thread per output row and four columns (one in the scalar
//            build), the neighbours' loads issued first, the adds in ascending k.  The backward pass gathers through the inverse
//            table nbr_bwd[K, n_in] in ascending FORWARD offset: no floating-point atomics, every result a pure function of the
//            inputs (MI355X: global float atomics run at a quarter of the plain-store rate and add in no fixed order).
//   global   one row per batch: a batch's rows (ascending row index, CSR `order` / `offsets`) are cut into chunks of
//            OSN_GPOOL_CHUNK; gpool_chunk_kernel gives a chunk to a workgroup, which reduces it in an order that depends on the
//            width alone; gpool_finish_kernel adds a batch's partials in chunk order.  A batch's bits depend on its own rows only.
//   broadcast  y[i] = x[i] (+ | *) g[batch(i)], streaming.
//
// Max: ties go to the first neighbour (local: lowest k; global: lowest row), +0 == -0, a NaN wins over every number and the
// first NaN stays.  All kernels are bandwidth-bound gathers or streams: wave64, 16-byte accesses when c % 4 == 0 and the
// pointers are 16-byte aligned, a scalar build otherwise.
#include "common.h"

namespace osn {

constexpr int GP_G = OSN_GPOOL_CHUNK;
constexpr int GP_SCAN_T = 1024;
enum { POOL_SUM = OSN_POOL_SUM, POOL_AVG = OSN_POOL_AVG, POOL_MAX = OSN_POOL_MAX };

template <int V, typename T>
__device__ inline void pl_ld(const T* __restrict__ p, T (&v)[V]) {
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
__device__ inline void pl_st(T* __restrict__ p, const T (&v)[V]) {
    if constexpr (V == 4) {
        *reinterpret_cast<uint4*>(p) = make_uint4(__builtin_bit_cast(uint32_t, v[0]), __builtin_bit_cast(uint32_t, v[1]),
                                                  __builtin_bit_cast(uint32_t, v[2]), __builtin_bit_cast(uint32_t, v[3]));
    } else {
        *p = v[0];
    }
}
// a table entry that names a row of [0, rows): -1 and anything else outside count as absent
__device__ inline bool pl_row_ok(int i, int64_t rows) { return uint64_t(uint32_t(i)) < uint64_t(rows); }

// local max, k ascending: the first neighbour, then anything greater; a NaN replaces a number and is never replaced
__device__ inline bool pl_take(float v, float best, int best_row) {
    return best_row < 0 || (!(best != best) && (v != v || v > best));
}
// global max, any order: NaN over numbers, greater over smaller, the lower row among equals (+0 == -0) and among NaNs
__device__ inline bool gp_better(float v, int r, float best, int best_row) {
    if (r < 0) return false;
    if (best_row < 0) return true;
    const bool vn = v != v, bn = best != best;
    if (vn || bn) return vn && (!bn || r < best_row);
    return v > best || (v == best && r < best_row);
}

// cnt[o] = present neighbours of output row o
__global__ __launch_bounds__(256) void pool_count_kernel(const int32_t* __restrict__ nbr, int64_t n_in, int64_t n_out, int K,
                                                         int32_t* __restrict__ cnt) {
    const int64_t o = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (o >= n_out) return;
    int m = 0;
    for (int k = 0; k < K; ++k) m += pl_row_ok(nbr[int64_t(k) * n_out + o], n_in) ? 1 : 0;
    cnt[o] = m;
}

// one thread per (output row, V columns); K = 8 (2^3) or 27 (3^3) offsets, unrolled
template <int V, int MODE, int K>
__global__ __launch_bounds__(256) void pool_fwd_kernel(const float* __restrict__ x, int64_t n_in, const int32_t* __restrict__ nbr,
                                                       int64_t n_out, int c, int cg, float* __restrict__ y,
                                                       int32_t* __restrict__ arg) {
    const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (e >= n_out * cg) return;
    const int64_t o = e / cg;
    const int col = int(e - o * cg) * V;
    float acc[V];
    int best[V];
#pragma unroll
    for (int u = 0; u < V; ++u) { acc[u] = 0.f; best[u] = -1; }
    int cnt = 0;
    int idx[K];
    float v[K][V];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int i = nbr[int64_t(j) * n_out + o];
        idx[j] = pl_row_ok(i, n_in) ? i : -1;
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {                       // every present neighbour's load, then the adds in order
        if (idx[j] >= 0) {
            pl_ld<V>(x + int64_t(idx[j]) * c + col, v[j]);
        } else {
#pragma unroll
            for (int u = 0; u < V; ++u) v[j][u] = 0.f;
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (idx[j] < 0) continue;
        ++cnt;
#pragma unroll
        for (int u = 0; u < V; ++u) {
            if (MODE == POOL_MAX) {
                if (pl_take(v[j][u], acc[u], best[u])) { acc[u] = v[j][u]; best[u] = idx[j]; }
            } else {
                acc[u] += v[j][u];
            }
        }
    }
    if (MODE == POOL_AVG) {
#pragma unroll
        for (int u = 0; u < V; ++u) acc[u] = cnt > 0 ? __fdiv_rn(acc[u], float(cnt)) : 0.f;
    }
    pl_st<V>(y + o * c + col, acc);
    if (MODE == POOL_MAX) pl_st<V>(arg + o * c + col, best);
}

// one thread per (input row, V columns): the terms of the forward offsets k = 0 .. K - 1 in that order; forward offset k is
// row K - 1 - k of the table when `flip` (the self map of an odd kernel is its own mirror)
template <int V, int MODE, int K>
__global__ __launch_bounds__(256) void pool_bwd_kernel(const float* __restrict__ gy, int64_t n_out, const int32_t* __restrict__ nbr_bwd,
                                                       int64_t n_in, int flip, int c, int cg, const int32_t* __restrict__ cnt,
                                                       const int32_t* __restrict__ arg, float* __restrict__ gx) {
    const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (e >= n_in * cg) return;
    const int64_t i = e / cg;
    const int col = int(e - i * cg) * V;
    float acc[V];
#pragma unroll
    for (int u = 0; u < V; ++u) acc[u] = 0.f;
    int idx[K], cn[K];
    float g[K][V];
    int a[K][V];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int r = flip ? K - 1 - j : j;
        const int o = nbr_bwd[int64_t(r) * n_in + i];
        idx[j] = pl_row_ok(o, n_out) ? o : -1;
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        cn[j] = 1;
#pragma unroll
        for (int u = 0; u < V; ++u) { g[j][u] = 0.f; a[j][u] = -1; }
        if (idx[j] >= 0) {
            pl_ld<V>(gy + int64_t(idx[j]) * c + col, g[j]);
            if (MODE == POOL_AVG) cn[j] = cnt[idx[j]];
            if (MODE == POOL_MAX) pl_ld<V>(arg + int64_t(idx[j]) * c + col, a[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (idx[j] < 0) continue;
#pragma unroll
        for (int u = 0; u < V; ++u) {
            if (MODE == POOL_SUM) acc[u] += g[j][u];
            else if (MODE == POOL_AVG) acc[u] += cn[j] > 0 ? __fdiv_rn(g[j][u], float(cn[j])) : 0.f;
            else if (int64_t(a[j][u]) == i) acc[u] += g[j][u];
        }
    }
    pl_st<V>(gx + i * c + col, acc);
}

// ---- global ---------------------------------------------------------------------------------------------------------------
__device__ inline void gp_range(const int64_t* __restrict__ offsets, int64_t b, int64_t n, int64_t& lo, int64_t& hi) {
    lo = offsets[b];
    hi = offsets[b + 1];
    lo = lo < 0 ? 0 : (lo > n ? n : lo);
    hi = hi < lo ? lo : (hi > n ? n : hi);
}

// chunk_base[b] = chunks of the batches before b, chunk_base[B] = all chunks.  One workgroup.
__global__ __launch_bounds__(GP_SCAN_T) void gpool_scan_kernel(const int64_t* __restrict__ offsets, int64_t B, int64_t n,
                                                               int64_t* __restrict__ chunk_base) {
    __shared__ int64_t sh[GP_SCAN_T];
    const int tid = threadIdx.x;
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 < B; b0 += GP_SCAN_T) {
        const int64_t b = b0 + tid;
        int64_t m = 0;
        if (b < B) {
            int64_t lo, hi;
            gp_range(offsets, b, n, lo, hi);
            m = (hi - lo + GP_G - 1) / GP_G;
        }
        sh[tid] = m;
        __syncthreads();
        for (int o = 1; o < GP_SCAN_T; o <<= 1) {
            const int64_t v = sh[tid] + (tid >= o ? sh[tid - o] : 0);
            __syncthreads();
            sh[tid] = v;
            __syncthreads();
        }
        if (b < B) chunk_base[b] = carry + sh[tid] - m;
        carry += sh[GP_SCAN_T - 1];
        __syncthreads();
    }
    if (tid == 0) chunk_base[B] = carry;
}

// The reduction state of one thread: V sums, or V (value, row) maxima.
template <int V, int MODE>
struct GpAcc {
    float v[V];
    int r[V];
    __device__ inline void init() {
#pragma unroll
        for (int u = 0; u < V; ++u) { v[u] = 0.f; r[u] = -1; }
    }
    __device__ inline void add(const float (&t)[V], int row) {
#pragma unroll
        for (int u = 0; u < V; ++u) {
            if (MODE == POOL_MAX) {
                if (gp_better(t[u], row, v[u], r[u])) { v[u] = t[u]; r[u] = row; }
            } else {
                v[u] += t[u];
            }
        }
    }
    __device__ inline void merge(const float (&t)[V], const int (&tr)[V]) {
#pragma unroll
        for (int u = 0; u < V; ++u) {
            if (MODE == POOL_MAX) {
                if (gp_better(t[u], tr[u], v[u], r[u])) { v[u] = t[u]; r[u] = tr[u]; }
            } else {
                v[u] += t[u];
            }
        }
    }
};

// rows e0 + lane, e0 + lane + step, ... < e1 of the list `order`, four loads in flight, taken in that order
template <int V, int MODE, bool MUL>
__device__ inline void gp_rows(GpAcc<V, MODE>& acc, const float* __restrict__ x, const float* __restrict__ x2, int64_t n, int c, int col,
                               const int32_t* __restrict__ order, int64_t e0, int64_t e1, int lane, int step) {
    for (int64_t j0 = e0 + lane; j0 < e1; j0 += 4 * int64_t(step)) {
        int row[4];
        float t[4][V], t2[4][V];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t j = j0 + int64_t(u) * step;
            const int i = j < e1 ? order[j] : -1;
            row[u] = pl_row_ok(i, n) ? i : -1;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (row[u] < 0) continue;
            pl_ld<V>(x + int64_t(row[u]) * c + col, t[u]);
            if (MUL) pl_ld<V>(x2 + int64_t(row[u]) * c + col, t2[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (row[u] < 0) continue;
            if (MUL) {
#pragma unroll
                for (int w = 0; w < V; ++w) t[u][w] = t[u][w] * t2[u][w];
            }
            acc.add(t[u], row[u]);
        }
    }
}

// one workgroup per chunk.  cg = column groups of V columns.  cg < 256: R = 256 / cg row lanes, lane r takes the chunk's rows
// r, r + R, ... in order, the lanes' states are merged in lane order.  cg >= 256: every thread takes whole column groups.
// MUL: the rows are x[i] * x2[i], formed as they are read (the pooled gradient of a broadcast multiplication).
template <int V, int MODE, bool MUL>
__global__ __launch_bounds__(256) void gpool_chunk_kernel(const float* __restrict__ x, const float* __restrict__ x2, int64_t n, int c,
                                                          int cg, const int32_t* __restrict__ order, const int64_t* __restrict__ offsets,
                                                          int64_t B, const int64_t* __restrict__ chunk_base, float* __restrict__ pval,
                                                          int32_t* __restrict__ prow) {
    __shared__ __attribute__((aligned(16))) float shv[256 * V];
    __shared__ __attribute__((aligned(16))) int shr[MODE == POOL_MAX ? 256 * V : V];
    const int tid = threadIdx.x;
    const int64_t chunk = blockIdx.x;
    if (chunk >= chunk_base[B]) return;
    int64_t lo = 0, hi = B - 1;                             // the batch b with chunk_base[b] <= chunk < chunk_base[b + 1]
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (chunk_base[mid + 1] <= chunk) lo = mid + 1;
        else hi = mid;
    }
    int64_t a, b;
    gp_range(offsets, lo, n, a, b);
    const int64_t e0 = a + (chunk - chunk_base[lo]) * GP_G;
    const int64_t e1 = e0 + GP_G < b ? e0 + GP_G : b;
    GpAcc<V, MODE> acc;
    if (cg >= 256) {
        for (int g = tid; g < cg; g += 256) {
            acc.init();
            gp_rows<V, MODE, MUL>(acc, x, x2, n, c, g * V, order, e0, e1, 0, 1);
            pl_st<V>(pval + chunk * c + g * V, acc.v);
            if (MODE == POOL_MAX) pl_st<V>(prow + chunk * c + g * V, acc.r);
        }
        return;
    }
    const int R = 256 / cg;
    const int r = tid / cg, g = tid - r * cg;
    acc.init();
    if (r < R) gp_rows<V, MODE, MUL>(acc, x, x2, n, c, g * V, order, e0, e1, r, R);
    pl_st<V>(shv + tid * V, acc.v);
    if (MODE == POOL_MAX) pl_st<V>(shr + tid * V, acc.r);
    __syncthreads();
    if (r != 0) return;
    for (int q = 1; q < R; ++q) {
        float t[V];
        int tr[V];
        pl_ld<V>(shv + (q * cg + g) * V, t);
        if (MODE == POOL_MAX) {
            pl_ld<V>(shr + (q * cg + g) * V, tr);
        } else {
#pragma unroll
            for (int u = 0; u < V; ++u) tr[u] = 0;
        }
        acc.merge(t, tr);
    }
    pl_st<V>(pval + chunk * c + g * V, acc.v);
    if (MODE == POOL_MAX) pl_st<V>(prow + chunk * c + g * V, acc.r);
}

// one thread per (batch, V columns): the batch's partials in ascending chunk order; avg: one division by float(n_b)
template <int V, int MODE>
__global__ __launch_bounds__(256) void gpool_finish_kernel(const int64_t* __restrict__ offsets, int64_t B, int64_t n,
                                                           const int64_t* __restrict__ chunk_base, int64_t max_chunks,
                                                           const float* __restrict__ pval, const int32_t* __restrict__ prow, int c, int cg,
                                                           float* __restrict__ y, int32_t* __restrict__ arg) {
    const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (e >= B * cg) return;
    const int64_t b = e / cg;
    const int col = int(e - b * cg) * V;
    int64_t k0 = chunk_base[b], k1 = chunk_base[b + 1];
    k0 = k0 < max_chunks ? k0 : max_chunks;
    k1 = k1 < max_chunks ? k1 : max_chunks;
    GpAcc<V, MODE> acc;
    acc.init();
    for (int64_t k = k0; k < k1; ++k) {
        float t[V];
        int tr[V];
        pl_ld<V>(pval + k * c + col, t);
        if (MODE == POOL_MAX) {
            pl_ld<V>(prow + k * c + col, tr);
        } else {
#pragma unroll
            for (int u = 0; u < V; ++u) tr[u] = 0;
        }
        acc.merge(t, tr);
    }
    if (MODE == POOL_AVG) {
        int64_t lo, hi;
        gp_range(offsets, b, n, lo, hi);
        const float nb = float(hi - lo);
#pragma unroll
        for (int u = 0; u < V; ++u) acc.v[u] = hi > lo ? __fdiv_rn(acc.v[u], nb) : 0.f;
    }
    if (MODE == POOL_MAX) {
#pragma unroll
        for (int u = 0; u < V; ++u)
            if (acc.r[u] < 0) acc.v[u] = -__builtin_inff();  // an empty batch
        pl_st<V>(arg + b * c + col, acc.r);
    }
    pl_st<V>(y + b * c + col, acc.v);
}

// gx[i] = gy[rank[i]]  |  gy[rank[i]] / float(n_b)  |  arg[rank[i]] == i ? gy[rank[i]] : 0.  Every element of gx is written.
template <int V, int MODE>
__global__ __launch_bounds__(256) void gpool_bwd_kernel(const float* __restrict__ gy, const int32_t* __restrict__ rank,
                                                        const int64_t* __restrict__ offsets, const int32_t* __restrict__ arg, int64_t n,
                                                        int64_t B, int c, int cg, float* __restrict__ gx) {
    const int64_t total = n * cg;
    for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
        const int64_t i = e / cg;
        const int col = int(e - i * cg) * V;
        const int b = rank[i];
        float g[V];
#pragma unroll
        for (int u = 0; u < V; ++u) g[u] = 0.f;
        if (pl_row_ok(b, B)) {
            pl_ld<V>(gy + int64_t(b) * c + col, g);
            if (MODE == POOL_AVG) {
                int64_t lo, hi;
                gp_range(offsets, b, n, lo, hi);
                const float nb = float(hi - lo);
#pragma unroll
                for (int u = 0; u < V; ++u) g[u] = hi > lo ? __fdiv_rn(g[u], nb) : 0.f;
            }
            if (MODE == POOL_MAX) {
                int a[V];
                pl_ld<V>(arg + int64_t(b) * c + col, a);
#pragma unroll
                for (int u = 0; u < V; ++u) g[u] = int64_t(a[u]) == i ? g[u] : 0.f;
            }
        }
        pl_st<V>(gx + i * c + col, g);
    }
}

// y[i] = x[i] + g[rank[i]]  (MUL: *)
template <int V, bool MUL>
__global__ __launch_bounds__(256) void broadcast_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                        const int32_t* __restrict__ rank, int64_t n, int64_t B, int c, int cg,
                                                        float* __restrict__ y) {
    const int64_t total = n * cg;
    for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
        const int64_t i = e / cg;
        const int col = int(e - i * cg) * V;
        const int b = rank[i];
        float a[V], t[V];
        pl_ld<V>(x + i * c + col, a);
#pragma unroll
        for (int u = 0; u < V; ++u) t[u] = MUL ? 1.f : 0.f;
        if (pl_row_ok(b, B)) pl_ld<V>(g + int64_t(b) * c + col, t);
#pragma unroll
        for (int u = 0; u < V; ++u) a[u] = MUL ? a[u] * t[u] : a[u] + t[u];
        pl_st<V>(y + i * c + col, a);
    }
}

struct GpoolWs {
    size_t base, pval, prow, total;
    int64_t max_chunks;
};
static GpoolWs gpool_ws(int64_t n, int64_t B, int c) {
    GpoolWs w;
    n = n > 0 ? n : 0;
    B = B > 0 ? B : 0;
    w.max_chunks = n / GP_G + (B < n ? B : n);              // full chunks, and at most one partial chunk per non-empty batch
    const size_t mc = size_t(w.max_chunks > 0 ? w.max_chunks : 1);
    const size_t cc = size_t(c > 0 ? c : 0);
    size_t o = 0;
    w.base = o; o += align_up(size_t(B + 1) * 8, 256);
    w.pval = o; o += align_up(mc * cc * 4, 256);
    w.prow = o; o += align_up(mc * cc * 4, 256);
    w.total = o;
    return w;
}

static int pl_blocks(int64_t work) {
    int64_t g = cdiv(work, 256);
    if (g > 8192) g = 8192;
    if (g < 1) g = 1;
    return int(g);
}

static bool pl_vec(int c, const void* a, const void* b = nullptr, const void* d = nullptr, const void* e = nullptr,
                   const void* f = nullptr) {
    return (c & 3) == 0 && aligned16(a) && aligned16(b) && aligned16(d) && aligned16(e) && aligned16(f);
}

constexpr int64_t PL_MAX_ROWS = (int64_t(1) << 31) - 1;
constexpr int64_t PL_MAX_THREADS = (int64_t(1) << 31) * 256 - 256;

// the chunked reduction behind osn_gpool_fwd and osn_broadcast_bwd_pooled (x2 != null: rows x * x2, sum only)
static int gpool_impl(const char* who, const float* x, const float* x2, int64_t n, int c, const int32_t* order, const int64_t* offsets,
                      int64_t B, int mode, float* y, int32_t* arg, void* ws, size_t ws_bytes, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(mode == POOL_SUM || mode == POOL_AVG || mode == POOL_MAX, OSN_E_ARG, "%s: mode %d (0 sum, 1 avg, 2 max)", who, mode);
    OSN_REQUIRE(n >= 0 && n <= PL_MAX_ROWS && B >= 0 && B <= PL_MAX_ROWS && c >= 1, OSN_E_ARG,
                "%s: need 0 <= n, n_batches < 2^31 and c >= 1 (n=%lld n_batches=%lld c=%d)", who, (long long)n, (long long)B, c);
    if (B == 0) return OSN_OK;
    const GpoolWs w = gpool_ws(n, B, c);
    OSN_REQUIRE(w.max_chunks <= PL_MAX_ROWS && B * int64_t(c) <= PL_MAX_THREADS, OSN_E_ARG, "%s: n_batches * c too large (%lld * %d)", who,
                (long long)B, c);
    OSN_REQUIRE(offsets && y && (mode != POOL_MAX || arg) && (n == 0 || (x && order)), OSN_E_ARG, "%s: null pointer", who);
    // (this family reports every refused argument, the workspace included, as OSN_E_ARG)
    OSN_REQUIRE(ws && aligned16(ws) && ws_bytes >= w.total, OSN_E_ARG, "%s: workspace too small (%zu < %zu)", who, ws_bytes, w.total);
    char* p = static_cast<char*>(ws);
    int64_t* chunk_base = reinterpret_cast<int64_t*>(p + w.base);
    float* pval = reinterpret_cast<float*>(p + w.pval);
    int32_t* prow = reinterpret_cast<int32_t*>(p + w.prow);
    const bool vec = pl_vec(c, x, x2, y, arg);
    const int cg = vec ? c / 4 : c;
    hipLaunchKernelGGL(gpool_scan_kernel, dim3(1), dim3(GP_SCAN_T), 0, st, offsets, B, n, chunk_base);
    const dim3 grid(unsigned(w.max_chunks)), fgrid(unsigned(cdiv(B * cg, 256))), block(256);
#define OSN_GPOOL_LAUNCH(V, M, MUL)                                                                                                  \
    do {                                                                                                                             \
        if (w.max_chunks > 0)                                                                                                        \
            hipLaunchKernelGGL((gpool_chunk_kernel<V, (M) == POOL_MAX ? POOL_MAX : POOL_SUM, MUL>), grid, block, 0, st, x, x2, n, c, cg, \
                               order, offsets, B, chunk_base, pval, prow);                                                           \
        hipLaunchKernelGGL((gpool_finish_kernel<V, M>), fgrid, block, 0, st, offsets, B, n, chunk_base, w.max_chunks, pval, prow, c, \
                           cg, y, arg);                                                                                              \
    } while (0)
    if (x2) {
        if (vec) OSN_GPOOL_LAUNCH(4, POOL_SUM, true);
        else OSN_GPOOL_LAUNCH(1, POOL_SUM, true);
    } else if (mode == POOL_SUM) {
        if (vec) OSN_GPOOL_LAUNCH(4, POOL_SUM, false);
        else OSN_GPOOL_LAUNCH(1, POOL_SUM, false);
    } else if (mode == POOL_AVG) {
        if (vec) OSN_GPOOL_LAUNCH(4, POOL_AVG, false);
        else OSN_GPOOL_LAUNCH(1, POOL_AVG, false);
    } else {
        if (vec) OSN_GPOOL_LAUNCH(4, POOL_MAX, false);
        else OSN_GPOOL_LAUNCH(1, POOL_MAX, false);
    }
#undef OSN_GPOOL_LAUNCH
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

}  // namespace osn

using namespace osn;

extern "C" int osn_pool_count(const int32_t* nbr, int64_t n_in, int64_t n_out, int K, int32_t* cnt, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(K == 8 || K == 27, OSN_E_ARG, "osn_pool_count: K=%d (8 = 2^3 or 27 = 3^3 offsets)", K);
    OSN_REQUIRE(n_in >= 0 && n_in <= PL_MAX_ROWS && n_out >= 0 && n_out <= PL_MAX_ROWS, OSN_E_ARG,
                "osn_pool_count: need 0 <= n_in, n_out < 2^31 (n_in=%lld n_out=%lld)", (long long)n_in, (long long)n_out);
    if (n_out == 0) return OSN_OK;
    OSN_REQUIRE(nbr && cnt, OSN_E_ARG, "osn_pool_count: null pointer");
    hipLaunchKernelGGL(pool_count_kernel, dim3(unsigned(cdiv(n_out, 256))), dim3(256), 0, st, nbr, n_in, n_out, K, cnt);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

#define OSN_POOL_BY_K(KERNEL, V, M, ...)                                                                       \
    do {                                                                                                       \
        if (K == 8) hipLaunchKernelGGL((KERNEL<V, M, 8>), grid, dim3(256), 0, st, __VA_ARGS__);                \
        else hipLaunchKernelGGL((KERNEL<V, M, 27>), grid, dim3(256), 0, st, __VA_ARGS__);                      \
    } while (0)
#define OSN_POOL_BY_MODE(KERNEL, V, ...)                                          \
    do {                                                                          \
        if (mode == POOL_SUM) OSN_POOL_BY_K(KERNEL, V, POOL_SUM, __VA_ARGS__);    \
        else if (mode == POOL_AVG) OSN_POOL_BY_K(KERNEL, V, POOL_AVG, __VA_ARGS__); \
        else OSN_POOL_BY_K(KERNEL, V, POOL_MAX, __VA_ARGS__);                     \
    } while (0)

extern "C" int osn_pool_fwd(const float* x, int64_t n_in, const int32_t* nbr, int64_t n_out, int K, int c, int mode, float* y,
                            int32_t* arg, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(K == 8 || K == 27, OSN_E_ARG, "osn_pool_fwd: K=%d (8 = 2^3 or 27 = 3^3 offsets)", K);
    OSN_REQUIRE(mode == POOL_SUM || mode == POOL_AVG || mode == POOL_MAX, OSN_E_ARG, "osn_pool_fwd: mode %d (0 sum, 1 avg, 2 max)", mode);
    OSN_REQUIRE(n_in >= 0 && n_in <= PL_MAX_ROWS && n_out >= 0 && n_out <= PL_MAX_ROWS && c >= 1 && n_out * int64_t(c) <= PL_MAX_THREADS,
                OSN_E_ARG, "osn_pool_fwd: need 0 <= n_in, n_out < 2^31 and c >= 1 (n_in=%lld n_out=%lld c=%d)", (long long)n_in,
                (long long)n_out, c);
    if (n_out == 0) return OSN_OK;
    OSN_REQUIRE(nbr && y && (x || n_in == 0) && (arg || mode != POOL_MAX), OSN_E_ARG, "osn_pool_fwd: null pointer");
    const bool vec = pl_vec(c, x, y, arg);
    const int cg = vec ? c / 4 : c;
    const dim3 grid(unsigned(cdiv(n_out * cg, 256)));
    if (vec) OSN_POOL_BY_MODE(pool_fwd_kernel, 4, x, n_in, nbr, n_out, c, cg, y, arg);
    else OSN_POOL_BY_MODE(pool_fwd_kernel, 1, x, n_in, nbr, n_out, c, cg, y, arg);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_pool_bwd(const float* gy, int64_t n_out, const int32_t* nbr_bwd, int64_t n_in, int K, int flip, int c, int mode,
                            const int32_t* cnt, const int32_t* arg, float* gx, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(K == 8 || K == 27, OSN_E_ARG, "osn_pool_bwd: K=%d (8 = 2^3 or 27 = 3^3 offsets)", K);
    OSN_REQUIRE(mode == POOL_SUM || mode == POOL_AVG || mode == POOL_MAX, OSN_E_ARG, "osn_pool_bwd: mode %d (0 sum, 1 avg, 2 max)", mode);
    OSN_REQUIRE(flip == 0 || flip == 1, OSN_E_ARG, "osn_pool_bwd: flip=%d (0 or 1)", flip);
    OSN_REQUIRE(n_in >= 0 && n_in <= PL_MAX_ROWS && n_out >= 0 && n_out <= PL_MAX_ROWS && c >= 1 && n_in * int64_t(c) <= PL_MAX_THREADS,
                OSN_E_ARG, "osn_pool_bwd: need 0 <= n_in, n_out < 2^31 and c >= 1 (n_in=%lld n_out=%lld c=%d)", (long long)n_in,
                (long long)n_out, c);
    if (n_in == 0) return OSN_OK;
    OSN_REQUIRE(nbr_bwd && gx && (gy || n_out == 0) && (cnt || mode != POOL_AVG || n_out == 0) && (arg || mode != POOL_MAX || n_out == 0),
                OSN_E_ARG, "osn_pool_bwd: null pointer");
    const bool vec = pl_vec(c, gy, gx, arg);
    const int cg = vec ? c / 4 : c;
    const dim3 grid(unsigned(cdiv(n_in * cg, 256)));
    if (vec) OSN_POOL_BY_MODE(pool_bwd_kernel, 4, gy, n_out, nbr_bwd, n_in, flip, c, cg, cnt, arg, gx);
    else OSN_POOL_BY_MODE(pool_bwd_kernel, 1, gy, n_out, nbr_bwd, n_in, flip, c, cg, cnt, arg, gx);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}
#undef OSN_POOL_BY_MODE
#undef OSN_POOL_BY_K

extern "C" size_t osn_gpool_ws_bytes(int64_t n, int64_t n_batches, int c) { return gpool_ws(n, n_batches, c).total; }

extern "C" int osn_gpool_fwd(const float* x, int64_t n, int c, const int32_t* order, const int64_t* offsets, int64_t n_batches, int mode,
                             float* y, int32_t* arg, void* ws, size_t ws_bytes, osn_stream_t stream) {
    return gpool_impl("osn_gpool_fwd", x, nullptr, n, c, order, offsets, n_batches, mode, y, arg, ws, ws_bytes, stream);
}

extern "C" int osn_gpool_bwd(const float* gy, const int32_t* rank, const int64_t* offsets, const int32_t* arg, int64_t n,
                             int64_t n_batches, int c, int mode, float* gx, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(mode == POOL_SUM || mode == POOL_AVG || mode == POOL_MAX, OSN_E_ARG, "osn_gpool_bwd: mode %d (0 sum, 1 avg, 2 max)", mode);
    OSN_REQUIRE(n >= 0 && n <= PL_MAX_ROWS && n_batches >= 0 && n_batches <= PL_MAX_ROWS && c >= 1, OSN_E_ARG,
                "osn_gpool_bwd: need 0 <= n, n_batches < 2^31 and c >= 1 (n=%lld n_batches=%lld c=%d)", (long long)n, (long long)n_batches, c);
    if (n == 0) return OSN_OK;
    OSN_REQUIRE(rank && gx && (n_batches == 0 || (gy && (offsets || mode != POOL_AVG) && (arg || mode != POOL_MAX))), OSN_E_ARG,
                "osn_gpool_bwd: null pointer");
    const bool vec = pl_vec(c, gy, gx, arg);
    const int cg = vec ? c / 4 : c;
    const dim3 grid(unsigned(pl_blocks(n * cg)));
#define OSN_GPOOL_BWD(V)                                                                                                                  \
    do {                                                                                                                                  \
        if (mode == POOL_SUM) hipLaunchKernelGGL((gpool_bwd_kernel<V, POOL_SUM>), grid, dim3(256), 0, st, gy, rank, offsets, arg, n, n_batches, c, cg, gx);      \
        else if (mode == POOL_AVG) hipLaunchKernelGGL((gpool_bwd_kernel<V, POOL_AVG>), grid, dim3(256), 0, st, gy, rank, offsets, arg, n, n_batches, c, cg, gx); \
        else hipLaunchKernelGGL((gpool_bwd_kernel<V, POOL_MAX>), grid, dim3(256), 0, st, gy, rank, offsets, arg, n, n_batches, c, cg, gx);                       \
    } while (0)
    if (vec) OSN_GPOOL_BWD(4);
    else OSN_GPOOL_BWD(1);
#undef OSN_GPOOL_BWD
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_broadcast_fwd(const float* x, const float* g, const int32_t* rank, int64_t n, int64_t n_batches, int c, int op,
                                 float* y, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(op == OSN_BROADCAST_ADD || op == OSN_BROADCAST_MUL, OSN_E_ARG, "osn_broadcast_fwd: op %d (0 add, 1 mul)", op);
    OSN_REQUIRE(n >= 0 && n <= PL_MAX_ROWS && n_batches >= 0 && n_batches <= PL_MAX_ROWS && c >= 1, OSN_E_ARG,
                "osn_broadcast_fwd: need 0 <= n, n_batches < 2^31 and c >= 1 (n=%lld n_batches=%lld c=%d)", (long long)n,
                (long long)n_batches, c);
    if (n == 0) return OSN_OK;
    OSN_REQUIRE(x && rank && y && (g || n_batches == 0), OSN_E_ARG, "osn_broadcast_fwd: null pointer");
    const bool vec = pl_vec(c, x, g, y);
    const int cg = vec ? c / 4 : c;
    const dim3 grid(unsigned(pl_blocks(n * cg)));
    if (vec && op) hipLaunchKernelGGL((broadcast_kernel<4, true>), grid, dim3(256), 0, st, x, g, rank, n, n_batches, c, cg, y);
    else if (vec) hipLaunchKernelGGL((broadcast_kernel<4, false>), grid, dim3(256), 0, st, x, g, rank, n, n_batches, c, cg, y);
    else if (op) hipLaunchKernelGGL((broadcast_kernel<1, true>), grid, dim3(256), 0, st, x, g, rank, n, n_batches, c, cg, y);
    else hipLaunchKernelGGL((broadcast_kernel<1, false>), grid, dim3(256), 0, st, x, g, rank, n, n_batches, c, cg, y);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_broadcast_bwd_pooled(const float* gy, const float* x, int64_t n, int c, const int32_t* order, const int64_t* offsets,
                                        int64_t n_batches, float* gg, void* ws, size_t ws_bytes, osn_stream_t stream) {
    return gpool_impl("osn_broadcast_bwd_pooled", gy, x, n, c, order, offsets, n_batches, POOL_SUM, gg, nullptr, ws, ws_bytes, stream);
}
