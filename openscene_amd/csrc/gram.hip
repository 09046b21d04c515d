// Second moments of point sets over a bank of scenes on gfx950: the Gram matrix  X^T X  of the (normalised) stored rows of
// every group of a CSR list of bank rows, rounded to fp16 as the query scores them -- a symmetric rank-k update whose
// contraction runs over the rows of the bank -- with the column sums of the same rounded rows.
//
//   osn_bank_gram / osn_bank_gram_fp8    h = fp16_rne(v * r), r = fp32 1 / (||v|| + 1e-5)  (run/evaluate.py:305,310 with its
//                                        .half()) or h = fp16_rne(v), v the stored row (fp16, or code * 2^e decoded exactly);
//                                        gram[g] = sum h h^T, sum[g] = sum h over the entries of group g, fp32
//
// A group is cut into slices of OSN_BANK_GRAM_SLICE consecutive entries (bank_chunk_scan_kernel numbers them).
// bank_scale_kernel (bank.h) writes one fp32 factor per entry (with normalize: one wave per row, the pool's reduction).  gram_kernel gives
// a workgroup one slice and one pair of 128-column tiles (ti <= tj): per step of 32 entries it loads the two column strips
// (16 / 8 bytes per lane and entry), multiplies by the entry's factor, rounds to fp16 and stages the strips ROW-MAJOR
// [entry][column] in LDS (two buffers, one barrier per step; the loads of four steps are in flight in a register ring).  The
// contraction runs over the entries, i.e. down the LDS rows, so BOTH operands are fetched transposed with
// ds_read_b64_tr_b16: lane i of a 16-lane group receives column i of four consecutive entries, two reads per 16 x 32
// fragment (wgrad_tl.hip's fragment; the order of the 32 entries inside a fragment is free as long as both operands use the
// same one, and rows 4 g + q, 16 + 4 g + q for lane group g keep a half-wave's two blocks on different banks with 288-byte
// rows).  Four waves as 2 x 2 over the tile, 4 x 4 blocks of v_mfma_f32_16x16x32_f16 per wave.  A diagonal tile also
// multiplies its fragments by a fragment of ones: the column sums, from the same h, through the same pipe.
// The tile is one fp32 partial in the workspace; gram_finish_kernel adds a group's partials in ascending slice order and
// writes an element and its mirror image from the same value.  No floating-point atomics: bitwise repeatable, symmetric,
// and a group's bits do not depend on its place in the list.
// An entry whose row lies outside the bank is skipped -- its loads are made from a clamped address (the first bytes of the
// bank) and not used, zeros are staged -- and recorded in the bank's err word (osn_bank_check).
#include "bank.h"
#include <type_traits>

namespace osn {

typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int G_S = OSN_BANK_GRAM_SLICE;
constexpr int G_T = 128;           // columns of a tile
constexpr int G_K = 32;            // entries of a step: the k of one MFMA
constexpr int G_D = 4;             // steps whose loads are in flight
constexpr int G_PITCH = G_T + 16;  // fp16 elements of an LDS row: 288 bytes = 72 dwords, 8 banks from row to row
static_assert(G_S % G_K == 0, "a slice is a whole number of steps");
static_assert(G_D % 2 == 0, "a step's LDS buffer is a constant of the unrolled ring");

// the pair (ti <= tj) number p of nt tile columns, pairs in row order: (0,0) (0,1) .. (0,nt-1) (1,1) ..
__device__ inline void gram_pair(int p, int nt, int& ti, int& tj) {
    ti = 0;
    while (p >= nt - ti) { p -= nt - ti; ++ti; }
    tj = ti + p;
}

// one workgroup per (slice, tile pair); the grid is dealt so that the pairs of a slice run on one XCD (one L2)
template <bool FP8, bool ROWS>
__global__ __launch_bounds__(256) void gram_kernel(const void* __restrict__ B, int64_t n, int d,
                                                   const int64_t* __restrict__ starts, int64_t G, const int64_t* __restrict__ rows,
                                                   int64_t L, const float* __restrict__ scale, const int64_t* __restrict__ slice_base,
                                                   int nt, int np, int64_t n_blocks, float* __restrict__ pgram,
                                                   float* __restrict__ psum, int32_t* __restrict__ pc, int32_t* __restrict__ err) {
    constexpr int RB = FP8 ? 1 : 2;
    typedef typename std::conditional<FP8, uint2, uint4>::type raw_t;      // 8 stored elements
    __shared__ __attribute__((aligned(16))) _Float16 img[2][2][G_K][G_PITCH];      // [buffer][strip][entry][column]
    __shared__ int cnt_sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    // blocks go to the XCDs round-robin: XCD x takes the logical blocks [x * per, (x + 1) * per)
    const int64_t per = (n_blocks + 7) >> 3;
    const int64_t blk = int64_t(blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if (blk >= n_blocks) return;
    const int64_t slice = blk / np;
    const int p = int(blk - slice * np);
    if (slice >= slice_base[G]) return;
    int ti, tj;
    gram_pair(p, nt, ti, tj);
    const bool diag = ti == tj;
    int64_t lo = 0, hi = G - 1;                             // the group g with slice_base[g] <= slice < slice_base[g + 1]
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (slice_base[mid + 1] <= slice) lo = mid + 1;
        else hi = mid;
    }
    int64_t a, b;
    bank_group_range(starts, lo, L, a, b);
    const int64_t e0 = a + (slice - slice_base[lo]) * G_S;
    const int64_t e1 = e0 + G_S < b ? e0 + G_S : b;
    const int steps = int((e1 - e0 + G_K - 1) / G_K);
    if (tid == 0) cnt_sh = 0;

    // staging: thread -> chunk sc of 8 columns and entries se, se + 16 of the step, in both strips
    const int sc = tid & 15, se = tid >> 4;
    const int colA = ti * G_T + sc * 8, colB = tj * G_T + sc * 8;
    const bool hasA = colA < d, hasB = colB < d;            // (a diagonal tile: strip B is strip A, loaded again from L1, not staged)
    const char* base = static_cast<const char*>(B);
    raw_t ra[G_D][2], rb[G_D][2];                           // a ring of G_D steps' loads: step t waits in slot t % G_D
    float fs[G_D][2];
    bool live[G_D][2];
    int cnt = 0;

    // the loads of step s.  Straight-line code -- every lane loads, a skipped entry, an entry past the slice and a column past d
    // from a clamped address (the first bytes of B, the slice's first entry), and stage() drops what it must not use -- so that
    // the loads of later steps stay in flight while an earlier step's are waited for
    auto fetch = [&](int s, int slot) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int64_t i = e0 + int64_t(s) * G_K + se + 16 * u;
            const bool in = i < e1;
            const int64_t ic = in ? i : e0;
            const int64_t r = ROWS ? rows[ic] : ic;
            const bool ok = in && r >= 0 && r < n;
            if (in && !ok && p == 0 && sc == 0) atomicOr(err, BANK_E_POOL_ROW);
            cnt += (ok && p == 0 && sc == 0) ? 1 : 0;
            const int64_t rr = ok ? r : 0;
            live[slot][u] = ok;
            fs[slot][u] = scale[ic];
            ra[slot][u] = *reinterpret_cast<const raw_t*>(base + (rr * d + (hasA ? colA : 0)) * RB);
            rb[slot][u] = *reinterpret_cast<const raw_t*>(base + (rr * d + (hasB ? colB : 0)) * RB);
        }
    };
    auto rounded = [&](const raw_t& raw, float s) -> half8 {   // fp16_rne(v * s) of 8 stored elements
        half8 v;
        if constexpr (FP8) {
            const half2 h0 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(raw.x, 1.0f, false);
            const half2 h1 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(raw.x, 1.0f, true);
            const half2 h2 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(raw.y, 1.0f, false);
            const half2 h3 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(raw.y, 1.0f, true);
            v = half8{h0[0], h0[1], h1[0], h1[1], h2[0], h2[1], h3[0], h3[1]};
        } else {
            v = __builtin_bit_cast(half8, raw);
        }
        return bank_round8(v, s);
    };
    auto stage = [&](int buf, int slot) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            half8 za = {}, zb = {};                         // (a skipped entry, padding: zeros, not 0 * v)
            if (live[slot][u] && hasA) za = rounded(ra[slot][u], fs[slot][u]);
            if (live[slot][u] && hasB) zb = rounded(rb[slot][u], fs[slot][u]);
            *reinterpret_cast<half8*>(&img[buf][0][se + 16 * u][sc * 8]) = za;
            if (!diag) *reinterpret_cast<half8*>(&img[buf][1][se + 16 * u][sc * 8]) = zb;
        }
    };

    f32x4 acc[4][4], accs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        accs[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    half8 ones;
#pragma unroll
    for (int k = 0; k < 8; ++k) ones[k] = (_Float16)1.0f;

    // (a slice holds at least one entry -- the scan gives a group ceil(length / slice) slices -- so e0 is a valid entry)
#pragma unroll
    for (int j = 0; j < G_D; ++j) fetch(j, j);              // (steps past the slice's end load clamped addresses: fetch)
    stage(0, 0);
    fetch(G_D, 0);
    __syncthreads();
    const int li = lane & 15, lg = lane >> 4;
    for (int s0 = 0; s0 < steps; s0 += G_D) {
#pragma unroll
        for (int j = 0; j < G_D; ++j) {                     // (unrolled: the ring's slots are registers)
            const int s = s0 + j;
            if (s < steps) {                                // (uniform over the workgroup, as is every branch around the reads below)
                const int buf = j & 1;                      // = s & 1: G_D is even
                // fragments by transpose reads: lane i of 16-lane group g points at (entry 4 g + (i >> 2), columns 4 (i & 3) .. + 3)
                // of a 16-column block and receives column i of entries 4 g .. 4 g + 3, then of 16 + 4 g .. 16 + 4 g + 3
                auto frag = [&](int strip, int c16) -> half8 {
                    const _Float16* q = &img[buf][strip][4 * lg + (li >> 2)][c16 + 4 * (li & 3)];
                    union { s16x4 h[2]; half8 v; } u;
                    u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(q));
                    u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(q + 16 * G_PITCH));
                    return u.v;
                };
                half8 fa[4], fb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) fa[i] = frag(0, wi * 64 + 16 * i);
#pragma unroll
                for (int i = 0; i < 4; ++i) fb[i] = frag(diag ? 0 : 1, wj * 64 + 16 * i);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[i][k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[i], fb[k], acc[i][k], 0, 0, 0);
                if (diag && wj == 0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) accs[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[i], ones, accs[i], 0, 0, 0);
                }
                stage(buf ^ 1, (j + 1) % G_D);              // the next step, whose loads were issued G_D steps ago
                fetch(s + 1 + G_D, (j + 1) % G_D);
                __syncthreads();
            }
        }
    }

    // partial[slice][pair][128][128]: C row = 4 (lane >> 4) + r (strip A's column), col = lane & 15 (strip B's column)
    float* out = pgram + blk * int64_t(G_T * G_T);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                out[(wi * 64 + 16 * i + 4 * lg + r) * G_T + wj * 64 + 16 * j + li] = acc[i][j][r];
    if (diag && wj == 0 && li == 0) {                       // every column of the ones product holds the sums
        float* so = psum + slice * int64_t(nt) * G_T + ti * G_T;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) so[wi * 64 + 16 * i + 4 * lg + r] = accs[i][r];
    }
    if (p == 0) {
        if (cnt) atomicAdd(&cnt_sh, cnt);                   // (integers: any order gives the same count)
        __syncthreads();
        if (tid == 0) pc[slice] = cnt_sh;
    }
}

// one thread per (group, tile pair, element): the group's partials in ascending slice order, written to (a, b) and (b, a)
__global__ __launch_bounds__(256) void gram_finish_kernel(const int64_t* __restrict__ slice_base, int64_t max_slices,
                                                          const float* __restrict__ pgram, const float* __restrict__ psum,
                                                          const int32_t* __restrict__ pc, int64_t G, int d, int nt, int np,
                                                          float* __restrict__ gram, float* __restrict__ sum,
                                                          int64_t* __restrict__ count) {
    constexpr int PER = G_T * G_T / 256;                    // workgroups of a tile
    const int64_t blk = blockIdx.x;
    const int64_t g = blk / (int64_t(np) * PER);
    if (g >= G) return;
    const int rem = int(blk - g * (int64_t(np) * PER));
    const int p = rem / PER;
    const int e = (rem - p * PER) * 256 + threadIdx.x;      // element of the tile
    int ti, tj;
    gram_pair(p, nt, ti, tj);
    int64_t k0 = slice_base[g], k1 = slice_base[g + 1];     // (clamped: bad starts were reported, nothing is read out of bounds)
    k0 = k0 < max_slices ? k0 : max_slices;
    k1 = k1 < max_slices ? k1 : max_slices;
    const float z = k1 > k0 ? -0.f : 0.f;                   // (an empty group gives +0; else -0 + x = x, a -0 included)
    const int ra = e / G_T, cb = e - ra * G_T;
    const int ca = ti * G_T + ra, cc = tj * G_T + cb;
    if (ca < d && cc < d && (ti != tj || ra <= cb)) {       // a diagonal tile: its upper triangle
        const float* src = pgram + int64_t(p) * (G_T * G_T) + e;
        const int64_t stride = int64_t(np) * (G_T * G_T);
        float s = z;
        int64_t k = k0;
        for (; k + 16 <= k1; k += 16) {                     // sixteen loads in flight, added in slice order
            float t[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) t[j] = src[(k + j) * stride];
#pragma unroll
            for (int j = 0; j < 16; ++j) s += t[j];
        }
        for (; k < k1; ++k) s += src[k * stride];
        float* o = gram + g * int64_t(d) * d;
        o[int64_t(ca) * d + cc] = s;
        o[int64_t(cc) * d + ca] = s;
    }
    if (ti == tj && ra == 0 && ca + cb < d) {               // the tile's 128 sums; the first of all also counts
        const int col = ca + cb;
        float s = z;
        for (int64_t k = k0; k < k1; ++k) s += psum[k * int64_t(nt) * G_T + col];
        sum[g * int64_t(d) + col] = s;
        if (col == 0) {
            int64_t m = 0;
            for (int64_t k = k0; k < k1; ++k) m += pc[k];
            count[g] = m;
        }
    }
}

struct GramWs {
    size_t base, scale, pgram, psum, pc, total;
    int64_t max_slices;
    int nt, np;
};
static GramWs gram_ws(int64_t G, int64_t L, int d) {
    GramWs w;
    G = G > 0 ? G : 0;
    L = L > 0 ? L : 0;
    d = d > 0 ? d : 0;
    w.nt = (d + G_T - 1) / G_T;
    w.np = w.nt * (w.nt + 1) / 2;
    w.max_slices = L / G_S + (G < L ? G : L);               // full slices, and at most one partial slice per non-empty group
    const size_t ms = size_t(w.max_slices > 0 ? w.max_slices : 1);
    size_t o = 0;
    w.base = o; o += align_up(size_t(G + 1) * 8, 256);
    w.scale = o; o += align_up(size_t(L > 0 ? L : 1) * 4, 256);
    w.pgram = o; o += align_up(ms * size_t(w.np) * G_T * G_T * 4, 256);
    w.psum = o; o += align_up(ms * size_t(w.nt) * G_T * 4, 256);
    w.pc = o; o += align_up(ms * 4, 256);
    w.total = o;
    return w;
}

}  // namespace osn

using namespace osn;

extern "C" size_t osn_bank_gram_ws_bytes(int64_t n_groups, int64_t n_entries, int d) { return gram_ws(n_groups, n_entries, d).total; }

// both entries: `bank` are fp16 rows or, with `fp8`, e4m3 codes that go with the row exponents `exps`; `who` names the entry in
// the messages
template <bool FP8>
static int bank_gram_impl(const char* who, const void* bank, const int8_t* exps, int64_t n, int d, const int64_t* starts,
                          int64_t n_groups, const int64_t* rows, int64_t n_entries, int normalize, float* gram, float* sum,
                          int64_t* count, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    constexpr int EL = FP8 ? 16 : 8;
    OSN_REQUIRE(n >= 0 && d >= EL && d % EL == 0 && d <= OSN_BANK_POOL_MAX_DIM, OSN_E_ARG,
                "%s: need n >= 0, d %% %d == 0 and d <= %d (n=%lld d=%d)", who, EL, OSN_BANK_POOL_MAX_DIM, (long long)n, d);
    OSN_REQUIRE(n_groups >= 0 && n_groups < (int64_t(1) << 31) && n_entries >= 0 && (normalize == 0 || normalize == 1), OSN_E_ARG,
                "%s: n_groups=%lld (0 .. 2^31 - 1) n_entries=%lld (>= 0) normalize=%d (0 or 1)", who, (long long)n_groups,
                (long long)n_entries, normalize);
    if (n_groups == 0) return OSN_OK;
    const GramWs w = gram_ws(n_groups, n_entries, d);
    const int64_t n_blocks = w.max_slices * w.np;
    const int64_t fin_blocks = n_groups * w.np * (G_T * G_T / 256);
    OSN_REQUIRE(n_blocks + 8 < (int64_t(1) << 31) && cdiv(n_entries, 4) < (int64_t(1) << 31), OSN_E_ARG,
                "%s: too many entries (%lld)", who, (long long)n_entries);
    OSN_REQUIRE(fin_blocks < (int64_t(1) << 31), OSN_E_ARG, "%s: n_groups * d * d too large (%lld groups, d=%d)", who,
                (long long)n_groups, d);                    // (the finish launch's grid: 256 elements of a tile per workgroup)
    OSN_REQUIRE(starts && gram && sum && count && err, OSN_E_ARG, "%s: null pointer", who);
    OSN_REQUIRE(n == 0 || (bank && aligned16(bank) && (exps || !FP8)), OSN_E_ARG,
                "%s: the bank's rows%s must be non-null, the rows 16-byte aligned", who, FP8 ? " and exponents" : "");
    OSN_REQUIRE(ws && aligned16(ws) && ws_bytes >= w.total, OSN_E_WS, "%s: workspace too small (%zu < %zu)", who, ws_bytes, w.total);
    char* p = static_cast<char*>(ws);
    int64_t* slice_base = reinterpret_cast<int64_t*>(p + w.base);
    float* scale = reinterpret_cast<float*>(p + w.scale);
    float* pgram = reinterpret_cast<float*>(p + w.pgram);
    float* psum = reinterpret_cast<float*>(p + w.psum);
    int32_t* pc = reinterpret_cast<int32_t*>(p + w.pc);
    hipLaunchKernelGGL(bank_chunk_scan_kernel<G_S>, dim3(1), dim3(BANK_SCAN_T), 0, st, starts, n_groups, n_entries, slice_base, err);
    if (w.max_slices > 0) {
        // an empty bank: every entry is out of range and skipped; the clamped loads still need readable bytes
        const void* B = n > 0 ? bank : static_cast<const void*>(pgram);
        hipLaunchKernelGGL((bank_scale_kernel<FP8>), dim3(unsigned(cdiv(n_entries, 4))), dim3(256), 0, st, B, exps, n, d, rows,
                           n_entries, normalize, scale);
        const dim3 grid(unsigned((n_blocks + 7) / 8 * 8)), block(256);
#define OSN_GRAM_LAUNCH(ROWS)                                                                                                  \
    hipLaunchKernelGGL((gram_kernel<FP8, ROWS>), grid, block, 0, st, B, n, d, starts, n_groups, rows, n_entries, scale, slice_base, \
                       w.nt, w.np, n_blocks, pgram, psum, pc, err)
        if (rows) OSN_GRAM_LAUNCH(true);
        else OSN_GRAM_LAUNCH(false);
#undef OSN_GRAM_LAUNCH
    }
    hipLaunchKernelGGL(gram_finish_kernel, dim3(unsigned(fin_blocks)), dim3(256), 0, st, slice_base, w.max_slices, pgram, psum, pc,
                       n_groups, d, w.nt, w.np, gram, sum, count);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_bank_gram(const void* bank_f16, int64_t n, int d, const int64_t* starts, int64_t n_groups, const int64_t* rows,
                             int64_t n_entries, int normalize, float* gram, float* sum, int64_t* count, int32_t* err, void* ws,
                             size_t ws_bytes, osn_stream_t stream) {
    return bank_gram_impl<false>("osn_bank_gram", bank_f16, nullptr, n, d, starts, n_groups, rows, n_entries, normalize, gram, sum,
                                 count, err, ws, ws_bytes, stream);
}

extern "C" int osn_bank_gram_fp8(const uint8_t* codes, const int8_t* exps, int64_t n, int d, const int64_t* starts, int64_t n_groups,
                                 const int64_t* rows, int64_t n_entries, int normalize, float* gram, float* sum, int64_t* count,
                                 int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream) {
    return bank_gram_impl<true>("osn_bank_gram_fp8", codes, exps, n, d, starts, n_groups, rows, n_entries, normalize, gram, sum,
                                count, err, ws, ws_bytes, stream);
}
