// Bank rows matched to exemplars on gfx950: for each of L bank rows the k most similar of M exemplar rows, without an L x M
// array anywhere.
//
//   osn_bank_unit_rows / _fp8    the operands of a row list as an fp16 image [M, d] (the exemplar side, prepared once)
//   osn_bank_match / _fp8        idx int32 [L, k], score float32 [L, k], count int32 [L]
//
// The contract (include/openscene_amd.h repeats it beside the entries):
//   operand  u = fp16_rne(v * r), r the fp32 factor of the row (bank.h: bank_row_factor, 1 / (||v|| + 1e-5) as
//            run/evaluate.py:305,310; fp8 rows decoded exactly, 2^e / (||c|| 2^e + 1e-5)), or u = fp16_rne(v) without normalize:
//            bit for bit the operand of osn_bank_gram (the same two functions of bank.h).
//   score    s(p, e) = the fp32 accumulation of the exact fp16 x fp16 products by v_mfma_f32_16x16x32_f16 over ceil(d / 32)
//            steps in ascending order, from a zero accumulator, zeros past d.  A lane's accumulator element depends on one
//            operand row of each side only: s is a function of the two rows and d, not of L, M, positions, k or the split.
//   order    one 64-bit key per candidate: the monotone 32-bit image of the score in the high word (a NaN: 0, below -inf's
//            0x007FFFFF; -0 is taken as +0), 0xFFFFFFFF - position in the low word.  The largest key is the best: equal
//            scores go to the lower position.  A key of 0 is "no candidate" (a real key's low word is at least 2^31).
//   result   a row's k largest keys in descending order; idx -1 and score -inf past count = min(k, M).
//
// The tile decision.  A workgroup (four waves) keeps a strip of M_TQ = 64 query rows RESIDENT in LDS over the whole of d --
// the operands are formed once while staging (one wave per row: load, factor, round, store), 64 x (d + 8) halves, 97 KB at
// d = 768 and 129 KB at d = 1024 of the 160 KB -- and STREAMS the exemplars: a wave takes 64 of a tile's M_TE = 256 exemplar
// columns and reads its B fragments (16 bytes per lane: eight consecutive k of one exemplar row) straight from the fp16
// image into registers, M_PF = 4 steps ahead in a ring that runs across tile ends.  Nothing is staged for the exemplars and
// the main loop has no barrier.  The alternative -- both sides streamed through LDS in k-steps under a 128 x 128
// accumulator tile -- forms the query operands again for every exemplar tile and pays a barrier per step; with the strip
// resident the contraction of a tile is one uninterrupted MFMA chain per wave (4 x 4 blocks of 16 x 16, 64 accumulator
// registers: a 64 x 64 wave tile, so that four ds_read_b128 and four global loads feed sixteen MFMAs), which is also what
// makes the score a pure function of the pair.  The strip allows one workgroup per CU, one wave per SIMD: latency is hidden
// inside the wave -- the query fragments of step s + 1 are read ahead of the MFMAs of step s -- and the whole register file
// (512 per lane) is the wave's.  DESIGN.md 4 gives the measured share of the roof and what binds.
// The fold.  After a tile's last step a lane holds 4 exemplar columns for each of its 16 query rows.  Each score becomes
// its 32-bit image and is compared with the high word of the row's current k-th key in LDS (it only ever grows, so a stale
// read only lets more through); the few that pass are inserted by a chain of 64-bit LDS integer maxima: slot j keeps the
// larger of (its key, the incoming key) and hands the smaller to slot j + 1.  Every slot is a maximum over what reaches it,
// so the k slots end as the k largest keys in order whatever the interleaving of lanes and waves: no lock, no barrier, no
// floating-point atomics.  For k = 1 that is one ds_max_u64 per passing candidate.
// The split.  The exemplar tiles are cut into `splits` contiguous ranges (grid y); every part writes its k keys per row to
// the workspace [splits][L][k] and match_merge_kernel keeps the k largest of a row's splits * k keys and decodes them.
// Keys are a total order over pure scores: the result does not depend on `splits`.
// Every load is unconditional from a clamped address (search.hip's rule): a query row past L or outside the bank reads
// the bank's first row and stages zeros (outside the bank: BANK_E_POOL_ROW in the err word); an exemplar column past M reads
// row M - 1 and never produces a key; a k group past d reads the row's first bytes and is replaced by zeros.
#include "bank.h"
#include <atomic>

namespace osn {

typedef unsigned long long u64;

constexpr int M_TQ = OSN_BANK_MATCH_TILE_Q;    // query rows of a workgroup
constexpr int M_TE = OSN_BANK_MATCH_TILE_E;    // exemplar columns of a tile: 64 per wave
constexpr int M_WJ = M_TE / 64;                // 16-column blocks of a wave
constexpr int M_K = 32;                        // the k of one MFMA step
constexpr int M_PF = 4;                        // steps whose exemplar loads are in flight
constexpr int M_MAXK = OSN_BANK_MATCH_MAX_K;
constexpr int M_FILL = 512;                    // workgroups the automatic split aims at: two per CU
constexpr int M_MAX_SPLITS = OSN_BANK_MATCH_MAX_SPLITS;
static_assert(M_TQ == 64 && M_TE == 256, "four waves: 4 x 4 blocks of 16 x 16 each");

__device__ __forceinline__ uint32_t match_image(float s) {
    uint32_t b = __float_as_uint(s);
    if (b == 0x80000000u) b = 0u;                                           // -0 ranks as +0
    const uint32_t m = b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    return s != s ? 0u : m;                                                 // a NaN below -inf (0x007FFFFF)
}
__device__ __forceinline__ float match_score(uint32_t m) {
    if (m == 0u) return __uint_as_float(0x7FC00000u);
    return __uint_as_float((m & 0x80000000u) ? (m ^ 0x80000000u) : ~m);
}

// one wave: the operands of bank row r (zeros when !ok; the loads are then made from row 0) to dst[0 .. d)
template <bool FP8, typename Dst>
__device__ __forceinline__ void match_operands(const void* __restrict__ B, const int8_t* __restrict__ E, int d, int64_t r, bool ok,
                                               int normalize, int lane, Dst* dst) {
    const int64_t rc = ok ? r : 0;
    const char* row = static_cast<const char*>(B) + rc * int64_t(d) * (FP8 ? 1 : 2);
    const float f = bank_row_factor<FP8>(row, d, FP8 ? bank_exp2(E[rc]) : 1.f, normalize, lane);
    const half8 zero = {};
    for (int grp = lane; grp < d / (FP8 ? 16 : 8); grp += 64) {
        const uint4 raw = *reinterpret_cast<const uint4*>(row + int64_t(grp) * 16);
        if (FP8) {
            half2 h[8];
            q8_widen(raw, h);
            const half8 v0 = {h[0][0], h[0][1], h[1][0], h[1][1], h[2][0], h[2][1], h[3][0], h[3][1]};
            const half8 v1 = {h[4][0], h[4][1], h[5][0], h[5][1], h[6][0], h[6][1], h[7][0], h[7][1]};
            *reinterpret_cast<half8*>(dst + grp * 16) = ok ? bank_round8(v0, f) : zero;
            *reinterpret_cast<half8*>(dst + grp * 16 + 8) = ok ? bank_round8(v1, f) : zero;
        } else {
            *reinterpret_cast<half8*>(dst + grp * 8) = ok ? bank_round8(__builtin_bit_cast(half8, raw), f) : zero;
        }
    }
}

// one wave per list entry: out[i] = the operands of bank row rows[i] (or i)
template <bool FP8>
__global__ __launch_bounds__(256) void unit_rows_kernel(const void* __restrict__ B, const int8_t* __restrict__ E, int64_t n, int d,
                                                        const int64_t* __restrict__ rows, int64_t M, int normalize,
                                                        _Float16* __restrict__ out, int32_t* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int64_t i = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (i >= M) return;
    const int64_t r = rows ? rows[i] : i;
    const bool ok = r >= 0 && r < n;
    if (!ok && lane == 0) atomicOr(err, BANK_E_POOL_ROW);
    match_operands<FP8>(B, E, d, r, ok, normalize, lane, out + i * int64_t(d));
}

template <bool FP8, bool ROWS>
__global__ __launch_bounds__(256) void match_kernel(const void* __restrict__ B, const int8_t* __restrict__ E, int64_t n, int d,
                                                    const int64_t* __restrict__ rows, int64_t L, int normalize,
                                                    const _Float16* __restrict__ X, int64_t M, int k, int64_t tiles_per_part,
                                                    u64* __restrict__ part_keys, int32_t* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) unsigned char match_lds[];
    u64* keys = reinterpret_cast<u64*>(match_lds);                                      // [M_TQ][M_MAXK], descending per row
    _Float16* strip = reinterpret_cast<_Float16*>(match_lds + M_TQ * M_MAXK * 8);       // [M_TQ][pitch]
    const int dpad = (d + M_K - 1) & ~(M_K - 1), pitch = dpad + 8;                      // (d + 8 halves: 4 banks from row to row)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q0 = int64_t(blockIdx.x) * M_TQ;
    const int64_t part = blockIdx.y;

    for (int i = tid; i < M_TQ * M_MAXK; i += 256) keys[i] = 0;
    for (int rr = wave; rr < M_TQ; rr += 4) {                                           // one wave per row, as the pool
        const int64_t i = q0 + rr;
        const bool in = i < L;
        const int64_t ic = in ? i : L - 1;
        const int64_t r = ROWS ? rows[ic] : ic;
        const bool ok = in && r >= 0 && r < n;
        if (in && !ok && lane == 0 && part == 0) atomicOr(err, BANK_E_POOL_ROW);
        _Float16* dst = strip + rr * pitch;
        match_operands<FP8>(B, E, d, r, ok, normalize, lane, dst);
        const half8 zero = {};
        for (int c = d + lane * 8; c < dpad; c += 512) *reinterpret_cast<half8*>(dst + c) = zero;
    }
    __syncthreads();

    const int li = lane & 15, lg = lane >> 4;
    const int steps = dpad / M_K;
    const int steps_pad = (steps + M_PF - 1) / M_PF * M_PF;    // a tile's steps in whole chunks of M_PF: step s waits in slot s % M_PF
    const int64_t n_et = (M + M_TE - 1) / M_TE;
    const int64_t t0 = part * tiles_per_part;
    const int64_t t1 = t0 + tiles_per_part < n_et ? t0 + tiles_per_part : n_et;
    if (t0 < t1) {
        f32x4 acc[4][M_WJ];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < M_WJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        half8 ring[M_PF][M_WJ];
        const _Float16* bp[M_WJ];                           // the lane's exemplar rows of the tile being fetched
        auto rows_of = [&](int64_t t) {                     // (a column past M: row M - 1, never a key)
#pragma unroll
            for (int j = 0; j < M_WJ; ++j) {
                const int64_t col = t * M_TE + wave * (16 * M_WJ) + 16 * j + li;
                bp[j] = X + (col < M ? col : M - 1) * int64_t(d);
            }
        };
        // straight-line loads, also past the part's end and past d (the row's first bytes, replaced by zeros when used)
        auto fetch = [&](int slot, int s) {
            const int kk = s * M_K + 8 * lg;
            const int ko = kk < d ? kk : 0;
#pragma unroll
            for (int j = 0; j < M_WJ; ++j) ring[slot][j] = *reinterpret_cast<const half8*>(bp[j] + ko);
        };
        auto insert = [&](int row, u64 x) {
            u64* slot = keys + row * M_MAXK;
            for (int j = 0; j < k && x != 0; ++j) {
                const u64 old = atomicMax(slot + j, x);
                x = old < x ? old : x;
            }
        };
        const half8 zero = {};
        // the query fragments of step s + 1 are read from the strip ahead of the MFMAs of step s (after a tile's last step: step 0
        // again -- the strip is the same for every tile), so that the LDS latency hides behind the matrix pipe
        const _Float16* sa = strip + li * pitch + 8 * lg;
        half8 a_cur[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a_cur[i] = *reinterpret_cast<const half8*>(sa + 16 * i * pitch);
        auto step = [&](int slot, int s) {
            const bool kin = s * M_K + 8 * lg < d;
            const int sn = s + 1 < steps ? s + 1 : 0;
            half8 a_nxt[4], b[M_WJ];
#pragma unroll
            for (int i = 0; i < 4; ++i) a_nxt[i] = *reinterpret_cast<const half8*>(sa + 16 * i * pitch + sn * M_K);
#pragma unroll
            for (int j = 0; j < M_WJ; ++j) b[j] = kin ? ring[slot][j] : zero;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < M_WJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_cur[i], b[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) a_cur[i] = a_nxt[i];
        };
        rows_of(t0);
#pragma unroll
        for (int j = 0; j < M_PF; ++j)
            if (j < steps) fetch(j, j);
        for (int64_t t = t0; t < t1; ++t) {
            for (int s0 = 0; s0 < steps_pad; s0 += M_PF) {
                // the chunk whose loads replace this one's: the next of the tile, or the first of the next tile
                const bool wrap = s0 + M_PF >= steps_pad;
                const int n0 = wrap ? 0 : s0 + M_PF;
                if (s0 + M_PF <= steps && n0 + M_PF <= steps && !wrap) {   // whole chunks: one basic block
#pragma unroll
                    for (int j = 0; j < M_PF; ++j) {        // (unrolled: the ring's slots are registers)
                        step(j, s0 + j);
                        fetch(j, n0 + j);
                    }
                } else {                                    // (every branch is uniform over the workgroup)
                    if (wrap) {
#pragma unroll
                        for (int j = 0; j < M_PF; ++j)
                            if (s0 + j < steps) step(j, s0 + j);
                        rows_of(t + 1);
#pragma unroll
                        for (int j = 0; j < M_PF; ++j)
                            if (j < steps) fetch(j, j);
                    } else {
#pragma unroll
                        for (int j = 0; j < M_PF; ++j) {
                            if (s0 + j < steps) step(j, s0 + j);
                            if (n0 + j < steps) fetch(j, n0 + j);
                        }
                    }
                }
            }
            // the fold: a lane's M_WJ columns of each of its 16 rows against the row's k-th key
            const int64_t c0 = t * M_TE + wave * (16 * M_WJ) + li;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * i + 4 * lg + r;
#pragma unroll
                    for (int j = 0; j < M_WJ; ++j) {        // (the k-th key is read again per block: the inserts before raise it)
                        const uint32_t kth = reinterpret_cast<const volatile uint32_t*>(keys + row * M_MAXK + (k - 1))[1];
                        const int64_t col = c0 + 16 * j;
                        const uint32_t m = match_image(acc[i][j][r]);
                        if (col < M && m >= kth) insert(row, (u64(m) << 32) | u64(0xFFFFFFFFu - uint32_t(col)));
                    }
                }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < M_WJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    __syncthreads();
    for (int i = tid; i < M_TQ * k; i += 256) {
        const int rr = i / k, s = i - rr * k;
        if (q0 + rr < L) part_keys[(part * L + q0 + rr) * k + s] = keys[rr * M_MAXK + s];
    }
}

// one thread per query row: the k largest of its splits * k keys, decoded
__global__ __launch_bounds__(256) void match_merge_kernel(const u64* __restrict__ part_keys, int64_t L, int k, int splits, int64_t M,
                                                          int32_t* __restrict__ idx, float* __restrict__ score,
                                                          int32_t* __restrict__ count) {
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= L) return;
    u64 best[M_MAXK];
#pragma unroll
    for (int u = 0; u < M_MAXK; ++u) best[u] = 0;
    for (int p = 0; p < splits; ++p)
        for (int s = 0; s < k; ++s) {
            u64 x = part_keys[(int64_t(p) * L + i) * k + s];
#pragma unroll
            for (int u = 0; u < M_MAXK; ++u) {
                const u64 hi = best[u] > x ? best[u] : x;
                x = best[u] > x ? x : best[u];
                best[u] = hi;
            }
        }
#pragma unroll
    for (int u = 0; u < M_MAXK; ++u)
        if (u < k) {
            const bool some = best[u] != 0;
            idx[i * k + u] = some ? int32_t(0xFFFFFFFFu - uint32_t(best[u])) : -1;
            score[i * k + u] = some ? match_score(uint32_t(best[u] >> 32)) : -INFINITY;
        }
    count[i] = int32_t(M < k ? M : k);
}

static int match_splits(int64_t L, int64_t M, int splits) {
    const int64_t n_qt = L > 0 ? cdiv(L, M_TQ) : 1, n_et = M > 0 ? cdiv(M, M_TE) : 1;
    if (splits <= 0) {                                      // fill the device; a part is at least one tile
        int64_t s = cdiv(M_FILL, n_qt);
        s = s < n_et ? s : n_et;
        return int(s < M_MAX_SPLITS ? s : M_MAX_SPLITS);
    }
    return splits < M_MAX_SPLITS ? splits : M_MAX_SPLITS;
}

constexpr size_t M_SPARE = 4096;   // readable bytes for the clamped loads of an empty bank

static size_t match_ws(int64_t L, int k, int splits) {
    return align_up(size_t(L > 0 ? L : 0) * size_t(k > 0 ? k : 0) * size_t(splits) * 8, 256) + M_SPARE;
}

}  // namespace osn

using namespace osn;

// what the four entries check of the bank and the row list, in the neighbouring entries' wording
template <bool FP8>
static int bank_args(const char* who, const void* bank, const int8_t* exps, int64_t n, int d, int64_t n_rows, int normalize,
                     const int32_t* err) {
    constexpr int EL = FP8 ? 16 : 8;
    OSN_REQUIRE(n >= 0 && d >= EL && d % EL == 0 && d <= OSN_BANK_POOL_MAX_DIM, OSN_E_ARG,
                "%s: need n >= 0, d %% %d == 0 and d <= %d (n=%lld d=%d)", who, EL, OSN_BANK_POOL_MAX_DIM, (long long)n, d);
    OSN_REQUIRE(n_rows >= 0 && n_rows < (int64_t(1) << 31) && (normalize == 0 || normalize == 1), OSN_E_ARG,
                "%s: n_rows=%lld (0 .. 2^31 - 1) normalize=%d (0 or 1)", who, (long long)n_rows, normalize);
    OSN_REQUIRE(err, OSN_E_ARG, "%s: null pointer", who);
    OSN_REQUIRE(n == 0 || (bank && aligned16(bank) && (exps || !FP8)), OSN_E_ARG,
                "%s: the bank's rows%s must be non-null, the rows 16-byte aligned", who, FP8 ? " and exponents" : "");
    return OSN_OK;
}

template <bool FP8>
static int unit_rows_impl(const char* who, const void* bank, const int8_t* exps, int64_t n, int d, const int64_t* rows, int64_t M,
                          int normalize, void* out, int32_t* err, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = bank_args<FP8>(who, bank, exps, n, d, M, normalize, err);
    if (rc != OSN_OK) return rc;
    if (M == 0) return OSN_OK;
    OSN_REQUIRE(out && aligned16(out), OSN_E_ARG, "%s: the image must be non-null and 16-byte aligned", who);
    // an empty bank: every row is outside it; the clamped loads read the image itself (M * d * 2 >= d bytes) and zeros are written
    const void* B = n > 0 ? bank : out;
    const int8_t* E = n > 0 ? exps : static_cast<const int8_t*>(out);
    hipLaunchKernelGGL((unit_rows_kernel<FP8>), dim3(unsigned(cdiv(M, 4))), dim3(256), 0, st, B, E, n, d, rows, M, normalize,
                       static_cast<_Float16*>(out), err);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_bank_unit_rows(const void* bank_f16, int64_t n, int d, const int64_t* rows, int64_t n_rows, int normalize,
                                  void* out_f16, int32_t* err, osn_stream_t stream) {
    return unit_rows_impl<false>("osn_bank_unit_rows", bank_f16, nullptr, n, d, rows, n_rows, normalize, out_f16, err, stream);
}

extern "C" int osn_bank_unit_rows_fp8(const uint8_t* codes, const int8_t* exps, int64_t n, int d, const int64_t* rows, int64_t n_rows,
                                      int normalize, void* out_f16, int32_t* err, osn_stream_t stream) {
    return unit_rows_impl<true>("osn_bank_unit_rows_fp8", codes, exps, n, d, rows, n_rows, normalize, out_f16, err, stream);
}

extern "C" size_t osn_bank_match_ws_bytes(int64_t n_rows, int64_t n_exemplars, int d, int k, int splits) {
    (void)d;
    return match_ws(n_rows, k, match_splits(n_rows, n_exemplars, splits));
}

template <bool FP8>
static int bank_match_impl(const char* who, const void* bank, const int8_t* exps, int64_t n, int d, const int64_t* rows, int64_t L,
                           int normalize, const void* exemplars, int64_t M, int k, int splits, int32_t* idx, float* score,
                           int32_t* count, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = bank_args<FP8>(who, bank, exps, n, d, L, normalize, err);
    if (rc != OSN_OK) return rc;
    OSN_REQUIRE(k >= 1 && k <= M_MAXK && M >= 1 && M < (int64_t(1) << 31) && splits >= 0 && splits <= M_MAX_SPLITS, OSN_E_ARG,
                "%s: k=%d (1 .. %d) n_exemplars=%lld (1 .. 2^31 - 1) splits=%d (0: chosen here, .. %d)", who, k, M_MAXK, (long long)M,
                splits, M_MAX_SPLITS);
    if (L == 0) return OSN_OK;
    OSN_REQUIRE(exemplars && aligned16(exemplars) && idx && score && count, OSN_E_ARG,
                "%s: null pointer, or the exemplar image is not 16-byte aligned", who);
    const int sp = match_splits(L, M, splits);
    const size_t need = match_ws(L, k, sp);
    OSN_REQUIRE(ws && aligned16(ws) && ws_bytes >= need, OSN_E_WS, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    char* spare = static_cast<char*>(ws) + (need - M_SPARE);
    const void* B = n > 0 ? bank : static_cast<const void*>(spare);
    const int8_t* E = n > 0 ? exps : reinterpret_cast<const int8_t*>(spare);
    const int64_t n_qt = cdiv(L, M_TQ), n_et = cdiv(M, M_TE);
    const int64_t per = cdiv(n_et, sp);
    const int dpad = (d + M_K - 1) / M_K * M_K;
    const size_t lds = size_t(M_TQ) * M_MAXK * 8 + size_t(M_TQ) * size_t(dpad + 8) * 2;
    constexpr int LDS_MAX = M_TQ * M_MAXK * 8 + M_TQ * (OSN_BANK_POOL_MAX_DIM + 8) * 2;
    int dev_id = 0;
    OSN_HIP(hipGetDevice(&dev_id));
    const bool dev_slot_ok = dev_id >= 0 && dev_id < 64;
    u64* part_keys = static_cast<u64*>(ws);
    // the dynamic-LDS opt-in (up to 133 KB): once per (instance, device); a part without that much LDS cannot run the kernel
#define OSN_MATCH_LAUNCH(ROWS)                                                                                              \
    do {                                                                                                                   \
        auto kern = match_kernel<FP8, ROWS>;                                                                               \
        static std::atomic<signed char> attr_set[64];                                                                      \
        if (!dev_slot_ok || !attr_set[dev_id].load(std::memory_order_relaxed)) {                                           \
            OSN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX)); \
            if (dev_slot_ok) attr_set[dev_id].store(1, std::memory_order_relaxed);                                         \
        }                                                                                                                  \
        hipLaunchKernelGGL(kern, dim3(unsigned(n_qt), unsigned(sp)), dim3(256), lds, st, B, E, n, d, rows, L, normalize,   \
                           static_cast<const _Float16*>(exemplars), M, k, per, part_keys, err);                            \
    } while (0)
    if (rows) OSN_MATCH_LAUNCH(true);
    else OSN_MATCH_LAUNCH(false);
#undef OSN_MATCH_LAUNCH
    hipLaunchKernelGGL(match_merge_kernel, dim3(unsigned(cdiv(L, 256))), dim3(256), 0, st, part_keys, L, k, sp, M, idx, score, count);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_bank_match(const void* bank_f16, int64_t n, int d, const int64_t* rows, int64_t n_rows, int normalize,
                              const void* exemplars_f16, int64_t n_exemplars, int k, int splits, int32_t* idx, float* score,
                              int32_t* count, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream) {
    return bank_match_impl<false>("osn_bank_match", bank_f16, nullptr, n, d, rows, n_rows, normalize, exemplars_f16, n_exemplars, k,
                                  splits, idx, score, count, err, ws, ws_bytes, stream);
}

extern "C" int osn_bank_match_fp8(const uint8_t* codes, const int8_t* exps, int64_t n, int d, const int64_t* rows, int64_t n_rows,
                                  int normalize, const void* exemplars_f16, int64_t n_exemplars, int k, int splits, int32_t* idx,
                                  float* score, int32_t* count, int32_t* err, void* ws, size_t ws_bytes, osn_stream_t stream) {
    return bank_match_impl<true>("osn_bank_match_fp8", codes, exps, n, d, rows, n_rows, normalize, exemplars_f16, n_exemplars, k,
                                 splits, idx, score, count, err, ws, ws_bytes, stream);
}
