// Descriptors of point sets over a bank of scenes on gfx950: the sum of the (normalised, weighted) stored rows of every group
// of a CSR list of bank rows -- a scene, an object of a heat-map, a user's selection -- in one gather-reduce pass.
//
//   osn_bank_pool / osn_bank_pool_fp8    sum[g] = sum over the entries i of group g of  w_i * v_i / (||v_i|| + 1e-5)
//                                        (run/evaluate.py:305, the normalisation the query scores with) or  w_i * v_i,
//                                        v_i the stored row (fp16, or code * 2^e decoded exactly), everything in fp32
//
// A group is cut into chunks of OSN_BANK_POOL_CHUNK consecutive entries; bank_chunk_scan_kernel (bank.h) numbers the chunks (one
// exclusive scan over the groups' chunk counts).  pool_kernel gives a chunk to a workgroup: wave w takes the chunk's entries w, w + 4, ...
// in order.  A wave owns a whole row: 16 bytes per lane and load group, the row stays in registers while the sum of squares is
// reduced across the wave (xor butterfly: every lane ends with the same bits), then the row is scaled and added into the lane's
// fp32 accumulators.  Four rows are in flight per wave.  The four waves add their accumulators through LDS in wave order into
// the chunk's partial in the workspace; pool_finish_kernel adds a group's partials in ascending chunk order.  No floating-point
// atomics: the result is a function of the input arrays alone, bitwise repeatable, and a group's bits do not depend on where
// the group stands in the list.
// An entry whose row lies outside the bank or whose weight is negative or not finite is skipped -- its rows[i] and weights[i] are
// read, its row loads are made from a clamped address (the first bytes of the bank) and not used -- and recorded in the bank's
// err word (osn_bank_check).
#include "bank.h"

namespace osn {

constexpr int P_C = OSN_BANK_POOL_CHUNK;
constexpr int P_U = 4;             // rows a wave has in flight
static_assert(P_C % 4 == 0, "a chunk is dealt to four waves");

// one workgroup per chunk.  FP8: rows are e4m3fn codes (16 per 16-byte load) with the exponents E, else fp16 (8 per load);
// NG = the 16-byte load groups a lane holds of a row (d <= 64 * NG * EL)
template <bool FP8, int NG>
__global__ __launch_bounds__(256) void pool_kernel(const void* __restrict__ B, const int8_t* __restrict__ E, int64_t n, int d,
                                                   const int64_t* __restrict__ starts, int64_t G, const int64_t* __restrict__ rows,
                                                   int64_t L, const float* __restrict__ weights, int normalize,
                                                   const int64_t* __restrict__ chunk_base, float* __restrict__ psum,
                                                   float* __restrict__ pw, int32_t* __restrict__ pc, int32_t* __restrict__ err) {
    constexpr int EL = FP8 ? 16 : 8;
    constexpr int RB = FP8 ? 1 : 2;                         // bytes of a stored element
    constexpr int W = NG * 64 * EL;                         // columns a wave covers
    __shared__ __attribute__((aligned(16))) float part[4][W];
    __shared__ float wsh[4];
    __shared__ int csh[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t chunk = blockIdx.x;
    if (chunk >= chunk_base[G]) return;
    int64_t lo = 0, hi = G - 1;                             // the group g with chunk_base[g] <= chunk < chunk_base[g + 1]
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (chunk_base[mid + 1] <= chunk) lo = mid + 1;
        else hi = mid;
    }
    int64_t a, b;
    bank_group_range(starts, lo, L, a, b);
    const int64_t e0 = a + (chunk - chunk_base[lo]) * P_C;
    const int64_t e1 = e0 + P_C < b ? e0 + P_C : b;
    const int ng = d / EL;
    const char* base = static_cast<const char*>(B);

    float acc[NG][EL];
#pragma unroll
    for (int j = 0; j < NG; ++j)
#pragma unroll
        for (int k = 0; k < EL; ++k) acc[j][k] = -0.f;      // (-0 + x = x for every x, a stored -0 included)
    float wacc = 0.f;
    int cnt = 0;
    for (int64_t i0 = e0 + wave; i0 < e1; i0 += 4 * P_U) {
        uint4 raw[P_U][NG];
        float w[P_U], sc[P_U];
        bool ok[P_U];
#pragma unroll
        for (int u = 0; u < P_U; ++u) {                     // everything below is uniform over the wave
            const int64_t i = i0 + 4 * u;
            const bool in = i < e1;
            const int64_t r = in ? (rows ? rows[i] : i) : 0;
            w[u] = (in && weights) ? weights[i] : 1.f;
            const bool bad_r = r < 0 || r >= n;
            const bool bad_w = !(w[u] >= 0.f && w[u] <= 3.402823466e38f);      // (NaN fails it too)
            if (in && lane == 0 && (bad_r || bad_w))
                atomicOr(err, (bad_r ? BANK_E_POOL_ROW : 0) | (bad_w ? BANK_E_POOL_WEIGHT : 0));
            ok[u] = in && !bad_r && !bad_w;
            const int64_t rr = ok[u] ? r : 0;               // a skipped entry loads from the first bytes of B, never used
            sc[u] = FP8 ? __uint_as_float(uint32_t(127 + int(E[rr])) << 23) : 1.f;      // 2^e
#pragma unroll
            for (int j = 0; j < NG; ++j) {
                const int grp = lane + 64 * j;
                const bool has = grp < ng;
                uint4 v = *reinterpret_cast<const uint4*>(base + (has ? (rr * d + int64_t(grp) * EL) * RB : 0));
                if (!has) v = make_uint4(0, 0, 0, 0);
                raw[u][j] = v;
            }
        }
#pragma unroll
        for (int u = 0; u < P_U; ++u) {
            if (!ok[u]) continue;
            float v[NG][EL];
#pragma unroll
            for (int j = 0; j < NG; ++j) {
                if (FP8) {
                    half2 h[8];
                    q8_widen(raw[u][j], h);
#pragma unroll
                    for (int k = 0; k < 8; ++k) { v[j][2 * k] = (float)h[k][0]; v[j][2 * k + 1] = (float)h[k][1]; }
                } else {
                    const half8 h = __builtin_bit_cast(half8, raw[u][j]);
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[j][k] = (float)h[k];
                }
            }
            float s = w[u] * sc[u];                         // (2^e: exact)
            if (normalize) {
                float ss = 0.f;
#pragma unroll
                for (int j = 0; j < NG; ++j)
#pragma unroll
                    for (int k = 0; k < EL; ++k) ss = fmaf(v[j][k], v[j][k], ss);
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
                s = s / (sqrtf(ss) * sc[u] + 1e-5f);        // w * 2^e / (||c|| * 2^e + 1e-5); fp16 rows: 2^e = 1
            }
#pragma unroll
            for (int j = 0; j < NG; ++j)
#pragma unroll
                for (int k = 0; k < EL; ++k) acc[j][k] = fmaf(s, v[j][k], acc[j][k]);
            wacc += w[u];
            ++cnt;
        }
    }
#pragma unroll
    for (int j = 0; j < NG; ++j)
#pragma unroll
        for (int k = 0; k < EL; k += 4)
            *reinterpret_cast<float4*>(&part[wave][(j * 64 + lane) * EL + k]) = make_float4(acc[j][k], acc[j][k + 1], acc[j][k + 2], acc[j][k + 3]);
    if (lane == 0) { wsh[wave] = wacc; csh[wave] = cnt; }
    __syncthreads();
    float* out = psum + chunk * int64_t(d);
    for (int c = tid * 4; c < d; c += 1024) {               // the waves' accumulators in wave order
        float4 t = *reinterpret_cast<const float4*>(&part[0][c]);
#pragma unroll
        for (int wv = 1; wv < 4; ++wv) {
            const float4 o = *reinterpret_cast<const float4*>(&part[wv][c]);
            t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
        }
        *reinterpret_cast<float4*>(out + c) = t;
    }
    if (tid == 0) {
        pw[chunk] = ((wsh[0] + wsh[1]) + wsh[2]) + wsh[3];
        pc[chunk] = csh[0] + csh[1] + csh[2] + csh[3];
    }
}

// one thread per (group, four columns): the group's partials in ascending chunk order
__global__ __launch_bounds__(256) void pool_finish_kernel(const int64_t* __restrict__ chunk_base, int64_t max_chunks,
                                                          const float* __restrict__ psum, const float* __restrict__ pw,
                                                          const int32_t* __restrict__ pc, int64_t G, int d4, float* __restrict__ sum,
                                                          float* __restrict__ wsum, int64_t* __restrict__ count) {
    const int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (idx >= G * d4) return;
    const int64_t g = idx / d4;
    const int c = int(idx - g * d4);
    int64_t k0 = chunk_base[g], k1 = chunk_base[g + 1];     // (clamped: bad starts were reported, nothing is read out of bounds)
    k0 = k0 < max_chunks ? k0 : max_chunks;
    k1 = k1 < max_chunks ? k1 : max_chunks;
    const float4* p = reinterpret_cast<const float4*>(psum) + c;
    const float z = k1 > k0 ? -0.f : 0.f;                   // (an empty group gives +0; else -0 + x = x, a stored -0 included)
    float4 s = make_float4(z, z, z, z);
    int64_t k = k0;
    for (; k + 8 <= k1; k += 8) {                           // eight loads in flight, added in chunk order
        float4 t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = p[(k + j) * d4];
#pragma unroll
        for (int j = 0; j < 8; ++j) { s.x += t[j].x; s.y += t[j].y; s.z += t[j].z; s.w += t[j].w; }
    }
    for (; k < k1; ++k) {
        const float4 t = p[k * d4];
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    reinterpret_cast<float4*>(sum)[idx] = s;
    if (c == 0) {
        float w = 0.f;
        int64_t m = 0;
        for (k = k0; k < k1; ++k) { w += pw[k]; m += pc[k]; }
        wsum[g] = w;
        count[g] = m;
    }
}

struct PoolWs {
    size_t base, psum, pw, pc, total;
    int64_t max_chunks;
};
static PoolWs pool_ws(int64_t G, int64_t L, int d) {
    PoolWs w;
    G = G > 0 ? G : 0;
    L = L > 0 ? L : 0;
    w.max_chunks = L / P_C + (G < L ? G : L);               // full chunks, and at most one partial chunk per non-empty group
    const size_t mc = size_t(w.max_chunks > 0 ? w.max_chunks : 1);
    size_t o = 0;
    w.base = o; o += align_up(size_t(G + 1) * 8, 256);
    w.psum = o; o += align_up(mc * size_t(d > 0 ? d : 0) * 4, 256);
    w.pw = o; o += align_up(mc * 4, 256);
    w.pc = o; o += align_up(mc * 4, 256);
    w.total = o;
    return w;
}

}  // namespace osn

using namespace osn;

extern "C" size_t osn_bank_pool_ws_bytes(int64_t n_groups, int64_t n_entries, int d) { return pool_ws(n_groups, n_entries, d).total; }

// both pools: `bank` are fp16 rows or, with `fp8`, e4m3 codes that go with the row exponents `exps`; `who` names the entry in
// the messages
template <bool FP8>
static int bank_pool_impl(const char* who, const void* bank, const int8_t* exps, int64_t n, int d, const int64_t* starts,
                          int64_t n_groups, const int64_t* rows, int64_t n_entries, const float* weights, int normalize, float* sum,
                          float* wsum, int64_t* count, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    constexpr int EL = FP8 ? 16 : 8;
    OSN_REQUIRE(n >= 0 && d >= EL && d % EL == 0 && d <= OSN_BANK_POOL_MAX_DIM, OSN_E_ARG,
                "%s: need n >= 0, d %% %d == 0 and d <= %d (n=%lld d=%d)", who, EL, OSN_BANK_POOL_MAX_DIM, (long long)n, d);
    OSN_REQUIRE(n_groups >= 0 && n_groups < (int64_t(1) << 31) && n_entries >= 0 && (normalize == 0 || normalize == 1), OSN_E_ARG,
                "%s: n_groups=%lld (0 .. 2^31 - 1) n_entries=%lld (>= 0) normalize=%d (0 or 1)", who, (long long)n_groups,
                (long long)n_entries, normalize);
    if (n_groups == 0) return OSN_OK;
    const PoolWs w = pool_ws(n_groups, n_entries, d);
    OSN_REQUIRE(w.max_chunks < (int64_t(1) << 31), OSN_E_ARG, "%s: too many entries (%lld)", who, (long long)n_entries);
    OSN_REQUIRE(cdiv(n_groups * (d / 4), 256) < (int64_t(1) << 31), OSN_E_ARG, "%s: n_groups * d too large (%lld * %d)", who,
                (long long)n_groups, d);                    // (the finish launch's grid: one thread per group and four columns)
    OSN_REQUIRE(starts && sum && wsum && count && err, OSN_E_ARG, "%s: null pointer", who);
    OSN_REQUIRE(aligned16(sum), OSN_E_ARG, "%s: sum must be 16-byte aligned", who);
    OSN_REQUIRE(n == 0 || (bank && aligned16(bank) && (exps || !FP8)), OSN_E_ARG,
                "%s: the bank's rows%s must be non-null, the rows 16-byte aligned", who, FP8 ? " and exponents" : "");
    OSN_REQUIRE(ws && aligned16(ws) && ws_bytes >= w.total, OSN_E_WS, "%s: workspace too small (%zu < %zu)", who, ws_bytes, w.total);
    char* p = static_cast<char*>(ws);
    int64_t* chunk_base = reinterpret_cast<int64_t*>(p + w.base);
    float* psum = reinterpret_cast<float*>(p + w.psum);
    float* pw = reinterpret_cast<float*>(p + w.pw);
    int32_t* pc = reinterpret_cast<int32_t*>(p + w.pc);
    hipLaunchKernelGGL(bank_chunk_scan_kernel<P_C>, dim3(1), dim3(BANK_SCAN_T), 0, st, starts, n_groups, n_entries, chunk_base, err);
    if (w.max_chunks > 0) {
        // an empty bank: every entry is out of range and skipped; the clamped loads still need 16 readable bytes
        const void* B = n > 0 ? bank : static_cast<const void*>(psum);
        const int8_t* E = n > 0 ? exps : reinterpret_cast<const int8_t*>(psum);
        const dim3 grid(unsigned(w.max_chunks)), block(256);
#define OSN_POOL_LAUNCH(NG)                                                                                                         \
    hipLaunchKernelGGL((pool_kernel<FP8, NG>), grid, block, 0, st, B, E, n, d, starts, n_groups, rows, n_entries, weights, normalize, \
                       chunk_base, psum, pw, pc, err)
        static_assert(OSN_BANK_POOL_MAX_DIM <= 64 * 2 * 8 && OSN_BANK_POOL_MAX_DIM <= 64 * 16, "load groups per lane: fp16 <= 2, fp8 1");
        if (FP8 || d <= 64 * EL) OSN_POOL_LAUNCH(1);
        else if constexpr (!FP8) OSN_POOL_LAUNCH(2);
#undef OSN_POOL_LAUNCH
    }
    const int d4 = d / 4;
    hipLaunchKernelGGL(pool_finish_kernel, dim3(unsigned(cdiv(n_groups * d4, 256))), dim3(256), 0, st, chunk_base, w.max_chunks, psum,
                       pw, pc, n_groups, d4, sum, wsum, count);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_bank_pool(const void* bank_f16, int64_t n, int d, const int64_t* starts, int64_t n_groups, const int64_t* rows,
                             int64_t n_entries, const float* weights, int normalize, float* sum, float* wsum, int64_t* count,
                             int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream) {
    return bank_pool_impl<false>("osn_bank_pool", bank_f16, nullptr, n, d, starts, n_groups, rows, n_entries, weights, normalize, sum,
                                 wsum, count, err, ws, ws_bytes, stream);
}

extern "C" int osn_bank_pool_fp8(const uint8_t* codes, const int8_t* exps, int64_t n, int d, const int64_t* starts, int64_t n_groups,
                                 const int64_t* rows, int64_t n_entries, const float* weights, int normalize, float* sum, float* wsum,
                                 int64_t* count, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream) {
    return bank_pool_impl<true>("osn_bank_pool_fp8", codes, exps, n, d, starts, n_groups, rows, n_entries, weights, normalize, sum,
                                wsum, count, err, ws, ws_bytes, stream);
}
