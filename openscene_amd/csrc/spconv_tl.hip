// Sparse 3-D convolution on gfx950, second generation: per-tile COMPACTED pair lists, weights held in
// registers, output tile accumulated in LDS, work-balanced tiles handed out dynamically.
//
// Function parity (not a port) with MinkowskiEngine's convolution kernels (SURVEY.md section 2.1,
// appendix C item 5):  out[o] = sum_k in[nbr[k,o]] @ W[k].
//
// Why this shape (measured): on a 2 cm indoor scene a voxel has 5.3 of its 27 neighbours,
// so an output-stationary register tile pads every 32-row group to ~2x the real work and re-stages the weight
// chunk of every (tile, offset, channel chunk) through LDS.  Here:
//   * the kernel map of a tile of output rows is stored per offset as a dense list of (input row, local output
//     row) pairs (osn_tile_lists_build), so the MFMAs only see real pairs (padded to 32 per (tile, offset));
//   * a tile-ordered table puts the rows with many neighbours last, and the slowest tile takes 8x the fastest
//     (phase timers, profiles/): the tiles are handed to persistent workgroups through one atomic counter,
//     densest first (longest job first), instead of one workgroup per tile in launch order;
//   * a workgroup = NW waves, one per 32 output columns; a wave keeps the split-bf16 B fragments of W[k] for
//     ITS columns in registers for a whole (tile, offset), so weights enter the CU once per (tile, offset), are
//     loaded by exactly one wave, and never touch LDS (the load path into a CU, 64 B/clk, is what the first
//     version of this kernel saturated);
//   * gathered rows are split into three bf16 pieces ONCE per workgroup while they are staged to LDS; all waves
//     read ready-made MFMA A fragments with ds_read_b128;
//   * the pair lists of a batch of offsets are brought into LDS with one round of loads and the (offset, chunk,
//     32-pair step) sequence runs as one flat software pipeline whose gathers are issued ahead across offset
//     boundaries;
//   * the 16 x 16 result blocks are added into an fp32 output tile in LDS at the pairs' local output rows.
//     Within one offset an output row occurs at most once, offsets are walked in ascending order with
//     workgroup barriers in between, and a workgroup owns its rows exclusively => no atomics on data, fixed
//     summation order: bitwise reproducible whichever workgroup draws which tile;
//   * the epilogue streams the tile to HBM through the `out_rows` permutation (features stay in the caller's
//     row order) and can emit the per-tile column sums / sums of squares the following batch norm needs.
// Arithmetic: "bf16x6" (split.h) -- three bf16 pieces per operand, six of the nine products accumulated in fp32 on
// v_mfma_f32_16x16x32_bf16: fp32-class accuracy.
#include "common.h"
#include <atomic>
#include <type_traits>
#include "weight_prep.h"
#include "split.h"
#include "epilogue.h"

namespace osn {

constexpr int TL_BMAX = 88;       // rows per tile at most (LDS budget of the 128-column instance, 2 workgroups / CU)
constexpr int TL_LIST_BMAX = 128; // rows per tile the LISTS can describe (a local row is 8 bits of a packed entry; spconv_pl.hip takes 128)
constexpr int TL_BMIN = 32;       // rows per tile of small tables
constexpr int TL_BOCC3 = 64;      // rows per tile that osn_tile_rows hands out at most (three workgroups per CU, see there)
constexpr int TL_LCAP = 1024;     // packed list entries resident in LDS per batch of offsets
constexpr int TL_STEPS = TL_LCAP / 32 * 4;   // step-table entries: 32-pair steps of a batch x channel chunks (<= 4: 512 channels)
constexpr int TL_KMAX = 128;      // kernel offsets a list-mode launch can take (5^3 = 125)
constexpr int TL_CIN_MAX = TL_STEPS / (TL_LCAP / 32) * 128;   // input channels the step table holds: its chunks of at most 4 x 32 channels
constexpr int64_t TL_ROWS_MAX = int64_t(1) << 24;             // input rows: a packed list entry keeps the row in 24 bits
constexpr int TL_SLOTS = 512;     // persistent workgroups per column group (2 per CU)
constexpr int TL_MAX_DEVICES = 64; // per-device "LDS opt-in done" flags of every kernel instance

// ---- layout of a tile-list buffer ("tl"): tiles of bm = osn_tile_rows(n_out) consecutive table rows
//   int32 cnt[n_tiles][K]        pairs per (tile, offset)                 (256-byte aligned)
//   int2  lst[n_tiles][K][bm]    (input row, local output row), valid pairs first, ascending local row
struct TlView {
    int32_t* cnt;
    int2* lst;
    int64_t nt;
    size_t bytes;
};

static TlView tl_view(const void* base, int64_t n_out, int K, int bm) {
    TlView v;
    char* p = static_cast<char*>(const_cast<void*>(base));
    v.nt = cdiv(n_out > 0 ? n_out : 1, bm);
    const size_t cb = align_up(size_t(v.nt) * K * 4, 256);
    v.cnt = reinterpret_cast<int32_t*>(p);
    v.lst = reinterpret_cast<int2*>(p ? p + cb : nullptr);
    v.bytes = cb + size_t(v.nt) * K * bm * 8;
    return v;
}

// ------------------------------------------------------------------------------------------- lists
// cnt / lst of every tile.  One wave per offset (k = wave, wave + 4, ...): ballot compaction, no barriers.
__global__ __launch_bounds__(256) void tile_lists_kernel(const int32_t* __restrict__ nbr, int64_t n_out, int K, int bm,
                                                         int32_t* __restrict__ cnt, int2* __restrict__ lst) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile = blockIdx.x;
    const int64_t row0 = tile * bm;
    const int rows = int(min(int64_t(bm), n_out - row0));
    for (int k = wave; k < K; k += 4) {
        int base = 0;
        int2* dst = lst + (tile * K + k) * bm;
        for (int j0 = 0; j0 < rows; j0 += 64) {
            const int j = j0 + lane;
            const int v = j < rows ? nbr[int64_t(k) * n_out + row0 + j] : -1;
            const bool ok = v >= 0;
            const unsigned long long m = __ballot(ok);
            if (ok) dst[base + __popcll(m & ((1ull << lane) - 1ull))] = make_int2(v, j);
            base += __popcll(m);
        }
        if (lane == 0) cnt[tile * K + k] = base;
    }
}

// ------------------------------------------------------------------------------------- weight prep
__global__ void weight_prep_tl_kernel(const float* __restrict__ W, int K, int cin, int cout, int flip_b, int64_t per_plane_f,
                                      int64_t per_plane_b, __bf16* __restrict__ Wf, __bf16* __restrict__ Wb) {
    const int64_t total = per_plane_f + per_plane_b;
    for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += int64_t(gridDim.x) * blockDim.x) {
        if (e < per_plane_f) weight_prep_tl_one(W, K, cin, cout, 0, 0, e, Wf);
        else weight_prep_tl_one(W, K, cin, cout, flip_b, 1, e - per_plane_f, Wb);
    }
}

// ------------------------------------------------------------------------------------------ conv
// PROF (tools only): wave 0 accumulates s_memtime deltas of the phases into prof[workgroup][10].
#define TL_TICK(slot)                                              \
    if (PROF) {                                                    \
        __builtin_amdgcn_sched_barrier(0);                         \
        const long long now_ = __builtin_amdgcn_s_memtime();       \
        tacc[slot] += now_ - tlast;                                \
        tlast = now_;                                              \
        __builtin_amdgcn_sched_barrier(0);                         \
    }

// 4 waves; wave w < NW owns output columns [32 w, 32 w + 32) of the workgroup's column group and BOTH 16-pair
// halves of a step (waves >= NW only help with the gathers and the staging); channel chunks of KS x 32 <= 128
// (B fragments of a chunk: KS k-steps x 2 column blocks x 3 planes = 24 KS VGPRs).  KS is the k-step count that
// tiles the input channels without a remainder where one exists (96 channels: KS = 3 -- with the fixed 128-channel
// chunk of round 2 a quarter of the weight-fragment loads and of the gather lanes of every 96-channel conv was padding).
// BUFG (full-chunk instances, feature matrices below 2 GB -- every launch of the benchmark configurations): the gathered rows come through
// a buffer resource over the feature matrix, like the weight fragments -- 32-bit offset row * (4 cin) + 4 col from one v_mad_u32_u24, the
// chunk's first channel in the scalar offset -- instead of a 64-bit multiply-add, two 64-bit adds and a channel clamp per quad (8 -> 2 VALU;
// round 5's A/B: step 8.80 -> 8.73 / 8.76 ms, bit-identical results, profiles/r05_s1_knobs_ab.txt).  Ragged chunks and matrices of 2 GB
// and more keep the 64-bit addresses.
// EPI (inference): the evaluation-mode batch norm of the stage in the epilogue (epilogue.h).  A template flag, not a run-time test: with
// the test in the training instances the 96 -> 96 kernel's spills went from 26 to 45 SGPRs and from 52 to 92 bytes of scratch per lane.
// The kernel's text is spconv_tl_kernel.h, included once per kernel template; per accumulator its products and their order are those of
// split_products() in split.h, for the template's piece count.
// the three-piece kernel, under the name and template parameters it always had ...
#define OSN_TL_TEMPLATE template <int NW, int KS, bool RAGGED, bool PROF = false, int OCC = 2, bool BUFG = false, bool EPI = false>
#define OSN_TL_NAME spconv_tl_kernel
#define OSN_TL_NP 3
#include "spconv_tl_kernel.h"
#undef OSN_TL_TEMPLATE
#undef OSN_TL_NAME
#undef OSN_TL_NP
// ... and the reduced inference modes: the same text with NP_ = 2 or 1 pieces (OCC and the tile height as the three-piece instance of
// the shape: fewer staged planes only leave LDS and registers unused)
#define OSN_TL_TEMPLATE template <int NP_, int NW, int KS, bool RAGGED, bool PROF, int OCC, bool BUFG, bool EPI>
#define OSN_TL_NAME spconv_tl_pieces_kernel
#define OSN_TL_NP NP_
#include "spconv_tl_kernel.h"
#undef OSN_TL_TEMPLATE
#undef OSN_TL_NAME
#undef OSN_TL_NP
#undef TL_TICK

// The kernel of a launch with `NP` pieces.  Reduced instances exist for the ragged launches and for the full-chunk launches that gather
// through a buffer resource (feature matrix below 2 GB: every launch of the U-Nets); a full-chunk launch on a larger matrix and the
// tools' PROF launches run the three-piece kernel in every mode (more exact than asked).
template <int NP, int NW, int KS, bool RAGGED, bool PROF, int OCC, bool BUFG, bool EPI>
static auto tl_kernel_of() {
    if constexpr (NP == 3 || PROF || !(RAGGED || BUFG)) return &spconv_tl_kernel<NW, KS, RAGGED, PROF, OCC, BUFG, EPI>;
    else return &spconv_tl_pieces_kernel<NP, NW, KS, RAGGED, false, OCC, BUFG, EPI>;
}


// (Round 4 also tried this convolution with the gathered rows brought into LDS by LDS-DMA (global_load_lds_dwordx4), one
// barrier per step, the bf16 split done by every MFMA wave on its own fragments and the weight fragments of the next
// (offset, chunk) prefetched into a second register set: three variants, 139 - 173 us against 145 - 159 us for the kernel above
// at the time, and 149 us with EVERY byte of memory traffic removed -- which is how the kernel turned out to be bound by
// instruction issue, not by memory or latency.  The experiment is commits f129c6a .. 7a3f559 of this repository; its measurements are
// profiles/r04_s2_*.  What came out of it is the instruction diet of spconv_tl_kernel above.)

static int tl_waves(int cout) {
    // waves (= 32-column groups) per workgroup: the width with the least padding, the wider one on ties
    int best = 1, best_pad = 1 << 30;
    for (int nw = 4; nw >= 1; --nw) {
        const int cw = 32 * nw;
        const int pad = int(cdiv(cout, cw)) * cw - cout;
        if (pad < best_pad) { best_pad = pad; best = nw; }
    }
    return best;
}

}  // namespace osn

using namespace osn;

extern "C" int osn_tile_rows(int64_t n_out) {
    // rows per tile: about two rounds of the persistent workgroups, a multiple of 8 between 32 and 64.  Round 4: at most 64 rows
    // (was 88) -- with the output tile in dynamic LDS a <= 64-row tile of <= 96 columns lets THREE workgroups share a CU (the
    // OCC = 3 instances: level-0 96 -> 96 133 -> 126 us, level-1 105 -> 99 us), and the instances that stay at two workgroups per CU
    // lose nothing (128 -> 96: 162 / 163 us at 88 / 64 rows)
    int64_t bm = cdiv(n_out > 0 ? n_out : 1, 2 * (TL_SLOTS / 2 * 3));
    bm = (bm + 7) / 8 * 8;
    if (bm < TL_BMIN) bm = TL_BMIN;
    if (bm > TL_BOCC3) bm = TL_BOCC3;
    return int(bm);
}

extern "C" size_t osn_tile_lists_bytes(int64_t n_out, int K, int bm) {
    if (K < 1 || bm < 1) return 256;
    return tl_view(nullptr, n_out, K, bm).bytes;
}

extern "C" int osn_tile_lists_build(const int32_t* nbr, int64_t n_out, int K, int bm, void* tl, osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(n_out >= 0 && n_out < (int64_t(1) << 31), OSN_E_ARG, "osn_tile_lists_build: n_out out of range");
    OSN_REQUIRE(K >= 1 && K <= TL_KMAX, OSN_E_ARG, "osn_tile_lists_build: K=%d (at most %d offsets)", K, TL_KMAX);
    OSN_REQUIRE(bm >= 1 && bm <= TL_LIST_BMAX, OSN_E_ARG, "osn_tile_lists_build: bm=%d (at most %d rows per tile)", bm, TL_LIST_BMAX);
    if (n_out == 0) return OSN_OK;
    OSN_REQUIRE(nbr && tl, OSN_E_ARG, "osn_tile_lists_build: null pointer");
    TlView v = tl_view(tl, n_out, K, bm);
    hipLaunchKernelGGL(tile_lists_kernel, dim3(unsigned(v.nt)), dim3(256), 0, st, nbr, n_out, K, bm, v.cnt, v.lst);
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" size_t osn_weight_prep_tl_bytes(int K, int cin, int cout, int for_dgrad) {
    const int nc = for_dgrad ? cout : cin, nn = for_dgrad ? cin : cout;
    return size_t(3) * size_t(K) * size_t((nc + 31) / 32) * size_t((nn + 15) / 16) * 1024;
}

extern "C" int osn_weight_prep_tl(const float* W, int K, int cin, int cout, int flip, void* Wp_fwd, void* Wp_dgrad,
                                  osn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(W && (Wp_fwd || Wp_dgrad) && K >= 1 && cin >= 1 && cout >= 1, OSN_E_ARG, "osn_weight_prep_tl: bad arguments");
    const int64_t ppf = Wp_fwd ? int64_t(K) * ((cin + 31) / 32) * ((cout + 15) / 16) * 512 : 0;
    const int64_t ppb = Wp_dgrad ? int64_t(K) * ((cout + 31) / 32) * ((cin + 15) / 16) * 512 : 0;
    int g = int(cdiv(ppf + ppb, 256));
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(weight_prep_tl_kernel, dim3(g), dim3(256), 0, st, W, K, cin, cout, flip, ppf, ppb,
                       static_cast<__bf16*>(Wp_fwd), static_cast<__bf16*>(Wp_dgrad));
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

// small tables: parts per tile such that a launch has ~1024 units of work (at most 16, at most K)
static int tl_split(int64_t n_out, int K, int cout, int bm) {
    if (K <= 1 || n_out <= 0) return 1;
    const int64_t units = cdiv(n_out, bm) * cdiv(cout, 32 * tl_waves(cout));
    int64_t nz = 1024 / (units > 0 ? units : 1);
    if (nz > 16) nz = 16;
    if (nz > K) nz = K;
    if (nz < 1) nz = 1;
    return int(nz);
}

// tile counters (one per column group; MUST be zero on entry, left dirty) + the partial tiles of a split launch
extern "C" size_t osn_spconv_fwd_tl_ws_bytes(int64_t n_out, int K, int cout, int bm) {
    if (bm < 1) return 512;
    const int nz = tl_split(n_out, K, cout, bm);
    return 512 + (nz > 1 ? size_t(nz) * size_t(n_out) * size_t(cout) * 4 : 0);
}

// out[out_rows ? out_rows[r] : r] = partial[0][r] + partial[1][r] + ...  (fixed order)
template <bool EPI>
__global__ void tl_reduce_parts_kernel(const float4* __restrict__ partial, int S, int64_t n_out, int c4,
                                       const int32_t* __restrict__ out_rows, float4* __restrict__ out, const Epi epi) {
    const int64_t total = n_out * c4;
    for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += int64_t(gridDim.x) * blockDim.x) {
        float4 s = partial[e];
        for (int z = 1; z < S; ++z) {
            const float4 v = partial[int64_t(z) * total + e];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        const int64_t r = e / c4, c = e - r * c4;
        const int64_t orow = out_rows ? int64_t(out_rows[r]) : r;
        if constexpr (EPI) s = epi_quad(epi, s, orow, int(4 * c), 4 * c4);     // evaluation-mode batch norm (epilogue.h)
        out[orow * c4 + c] = s;
    }
}

// routing limit of the tile-list kernel (n_in = 0: a shape asked about before its rows are known).  Narrower than what
// osn_spconv_fwd_tl accepts: cin >= 8 where the entry takes 4, and the channel limit stated up front where the entry finds it in its
// step-table check
extern "C" int osn_spconv_fwd_tl_ok(int64_t n_in, int K, int cin, int cout) {
    return K >= 1 && K <= TL_KMAX && cin >= 8 && cin <= TL_CIN_MAX && (cin & 3) == 0 && cout >= 4 && (cout & 3) == 0 && n_in >= 0 &&
           n_in <= TL_ROWS_MAX;
}

static int spconv_fwd_tl_impl(const float* in, int64_t n_in, const void* Wp, const void* tl, const int32_t* out_rows,
                              float* out, double* bn_partial, int64_t n_out, int K, int cin, int cout, int bm, void* ws,
                              size_t ws_bytes, int32_t* counters, long long* prof, osn_stream_t stream, const Epi& epi = epi_none(),
                              int pieces = 3) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(pieces >= 1 && pieces <= 3, OSN_E_ARG, "osn_spconv_fwd_tl: pieces=%d (1, 2 or 3)", pieces);
    OSN_REQUIRE(n_out >= 0 && n_out < (int64_t(1) << 31), OSN_E_ARG, "osn_spconv_fwd_tl: n_out out of range");
    OSN_REQUIRE(K >= 1 && K <= TL_KMAX && cin >= 4 && (cin & 3) == 0 && cout >= 4 && (cout & 3) == 0, OSN_E_ARG,
                "osn_spconv_fwd_tl: needs K <= %d, cin %% 4 == 0, cout %% 4 == 0 (K=%d cin=%d cout=%d)", TL_KMAX, K, cin, cout);
    OSN_REQUIRE(bm >= 1 && bm <= TL_BMAX, OSN_E_ARG, "osn_spconv_fwd_tl: bm=%d (at most %d rows per tile)", bm, TL_BMAX);
    OSN_REQUIRE(n_in >= 0 && n_in <= TL_ROWS_MAX, OSN_E_RANGE,
                "osn_spconv_fwd_tl: %lld input rows (the kernel packs an input row into 24 bits; use osn_spconv_fwd_x6)", (long long)n_in);
    if (n_out == 0) return OSN_OK;
    OSN_REQUIRE(in && Wp && out, OSN_E_ARG, "osn_spconv_fwd_tl: null pointer");
    OSN_REQUIRE(tl || (K == 1 && !out_rows), OSN_E_ARG, "osn_spconv_fwd_tl: tile lists may be null only for K == 1 (identity map)");
    OSN_REQUIRE(aligned16(in) && aligned16(Wp) && aligned16(out), OSN_E_ARG, "osn_spconv_fwd_tl: pointers must be 16-byte aligned");
    const int nw = tl_waves(cout);
    const int gy = int(cdiv(cout, 32 * nw));
    const int nz = tl ? tl_split(n_out, K, cout, bm) : 1;
    const size_t need = osn_spconv_fwd_tl_ws_bytes(n_out, tl ? K : 1, cout, bm);
    OSN_REQUIRE(ws && ws_bytes >= need && gy <= 64, OSN_E_WS, "osn_spconv_fwd_tl: workspace %zu < %zu (or more than 64 column groups)", ws_bytes, need);
    OSN_REQUIRE(!(bn_partial && nz > 1), OSN_E_ARG, "osn_spconv_fwd_tl: bn_partial is not available on split (small-table) launches");
    int32_t* counter = counters;
    if (!counter) {                                  // no persistent counters: the head of the workspace, zeroed here
        OSN_HIP(hipMemsetAsync(ws, 0, 512, st));
        counter = static_cast<int32_t*>(ws);
    }
    const int self_reset = counters ? 1 : 0;
    float* partial = reinterpret_cast<float*>(static_cast<char*>(ws) + 512);
    const int32_t* cnt = nullptr;
    const int2* lst = nullptr;
    const int64_t n_tiles = cdiv(n_out, bm);
    if (tl) {
        TlView v = tl_view(tl, n_out, K, bm);
        cnt = v.cnt; lst = v.lst;
    }
    const int ns = (cin + 31) / 32, ncb = (cout + 15) / 16;
    const int64_t units = n_tiles * nz;
    unsigned gx = unsigned(units < TL_SLOTS ? units : TL_SLOTS);
    dim3 grid(gx, unsigned(gy));
    const bf16x8* wp = static_cast<const bf16x8*>(Wp);
    // k-steps per channel chunk: the whole contraction when it fits (<= 4 k-steps), else the divisor of the k-step count
    // that leaves no padded chunk (192 channels: 2 x 3), else 4
    const int ks = ns <= 4 ? ns : (ns % 4 == 0 ? 4 : (ns % 3 == 0 ? 3 : 4));
    OSN_REQUIRE(cdiv(ns, ks) * (TL_LCAP / 32) <= TL_STEPS, OSN_E_RANGE,
                "osn_spconv_fwd_tl: %d input channels need more than %d channel chunks per list batch (the kernel's step table); "
                "use osn_dense_fwd (K == 1) or osn_spconv_fwd_x6", cin, TL_STEPS / (TL_LCAP / 32));
    const bool ragged = (cin & 31) != 0 || ns % ks != 0;
    const bool ragged_host = ragged;
    const int ks_host = ks;
    // dynamic LDS = the output tile; beyond 64 KB per workgroup in total the kernel needs the opt-in attribute (once per instance)
    const size_t tile_bytes = size_t(bm + 1) * size_t(32 * nw + 4) * 4;
    // three workgroups per CU when the tile is low enough (<= 64 rows at <= 96 output columns: 3 x 53.7 KB)
    const bool occ3 = !prof && !ragged_host && nw <= 3 && ks_host <= 3 && tile_bytes + 28 * 1024 <= 54 * 1024;
    // gathers through a buffer resource (full-chunk instances, feature matrices below 2 GB)
    const uint64_t in_bytes64 = uint64_t(n_in) * uint64_t(cin) * 4u;
    // (the gather offset is __umul24(row, 4 cin): both factors below 2^24 -- rows by the check above, 4 cin stated here so that a
    //  later relaxation of either limit cannot silently corrupt addresses)
    const bool bufg = !prof && !ragged_host && in_bytes64 < (uint64_t(1) << 31) && n_in < (int64_t(1) << 24) && int64_t(4) * cin < (int64_t(1) << 24);
    const unsigned in_bytes = bufg ? unsigned(in_bytes64) : 0u;
    int rc_attr = OSN_OK;
    int dev_id = 0;
    OSN_HIP(hipGetDevice(&dev_id));
    const bool dev_slot_ok = dev_id >= 0 && dev_id < TL_MAX_DEVICES;      // (beyond: the attribute is set on every tall launch)
    const int dev_slot = dev_slot_ok ? dev_id : 0;
    if (occ3) {                                       // three persistent workgroups per CU
        gx = unsigned(units < TL_SLOTS / 2 * 3 ? units : TL_SLOTS / 2 * 3);
        grid = dim3(gx, unsigned(gy));
    }
    const bool use_epi = epi.mean != nullptr && nz == 1;        // (split launches: the reduction of the parts applies it)
#define OSN_TL4(NW_, KS_, RG_, PF_, OC_) OSN_TL5(NW_, KS_, RG_, PF_, OC_, false)
#define OSN_TL5(NW_, KS_, RG_, PF_, OC_, BG_)                                                                              \
    do {                                                                                                                   \
        if (use_epi) OSN_TL6(NW_, KS_, RG_, PF_, OC_, BG_, true);                                                          \
        else OSN_TL6(NW_, KS_, RG_, PF_, OC_, BG_, false);                                                                 \
    } while (0)
#define OSN_TL6(NW_, KS_, RG_, PF_, OC_, BG_, EP_)                                                                         \
    do {                                                                                                                   \
        if (pieces == 3) OSN_TL7(3, NW_, KS_, RG_, PF_, OC_, BG_, EP_);                                                    \
        else if (pieces == 2) OSN_TL7(2, NW_, KS_, RG_, PF_, OC_, BG_, EP_);                                               \
        else OSN_TL7(1, NW_, KS_, RG_, PF_, OC_, BG_, EP_);                                                                \
    } while (0)
#define OSN_TL7(NP_, NW_, KS_, RG_, PF_, OC_, BG_, EP_)                                                                    \
    do {                                                                                                                   \
        auto kern = tl_kernel_of<NP_, NW_, KS_, RG_, PF_, OC_, BG_, EP_>();                                                \
        /* dynamic LDS beyond the default limit needs the opt-in attribute: once per (instance, DEVICE), the largest tile any   \
           launch can ask for; relaxed atomics: a racing second thread (autograd's, the map prefetcher's) sets it again */       \
        static std::atomic<unsigned char> attr_set[TL_MAX_DEVICES];                                                        \
        if (tile_bytes > 36 * 1024 && !(dev_slot_ok && attr_set[dev_slot].load(std::memory_order_relaxed))) {              \
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,       \
                                    int(size_t(TL_BMAX + 1) * size_t(32 * NW_ + 4) * 4)) != hipSuccess) {                  \
                rc_attr = OSN_E_HIP;                                                                                       \
                break;                                                                                                     \
            }                                                                                                              \
            if (dev_slot_ok) attr_set[dev_slot].store(1, std::memory_order_relaxed);                                       \
        }                                                                                                                  \
        hipLaunchKernelGGL(kern, grid, dim3(256), tile_bytes, st, in, wp, cnt, lst, out_rows, out, bn_partial, counter, partial, nz, \
                           int(n_out), K, cin, cout, bm, int(n_tiles), ns, ncb, self_reset, prof, in_bytes,                \
                           use_epi ? epi : epi_none());                                                                    \
    } while (0)
#define OSN_TL3(NW_, KS_, RG_, PF_) OSN_TL4(NW_, KS_, RG_, PF_, 2)
#define OSN_TL2(NW_, KS_)                                                                                                  \
    do {                                                                                                                   \
        if (prof) {                                                                                                        \
            if (ragged) OSN_TL3(NW_, KS_, true, true);                                                                     \
            else OSN_TL3(NW_, KS_, false, true);                                                                           \
        } else if (ragged) {                                                                                               \
            OSN_TL3(NW_, KS_, true, false);                                                                                \
        } else if (occ3 && NW_ <= 3 && KS_ <= 3) {                                                                         \
            if (bufg) OSN_TL5((NW_ <= 3 ? NW_ : 3), (KS_ <= 3 ? KS_ : 3), false, false, 3, true);                          \
            else OSN_TL4((NW_ <= 3 ? NW_ : 3), (KS_ <= 3 ? KS_ : 3), false, false, 3);                                     \
        } else {                                                                                                           \
            if (bufg) OSN_TL5(NW_, KS_, false, false, 2, true);                                                            \
            else OSN_TL3(NW_, KS_, false, false);                                                                          \
        }                                                                                                                  \
    } while (0)
#define OSN_TL(NW_)                                                                                                        \
    do {                                                                                                                   \
        switch (ks) {                                                                                                      \
            case 1: OSN_TL2(NW_, 1); break;                                                                                \
            case 2: OSN_TL2(NW_, 2); break;                                                                                \
            case 3: OSN_TL2(NW_, 3); break;                                                                                \
            default: OSN_TL2(NW_, 4); break;                                                                               \
        }                                                                                                                  \
    } while (0)
    switch (nw) {
        case 4: OSN_TL(4); break;
        case 3: OSN_TL(3); break;
        case 2: OSN_TL(2); break;
        default: OSN_TL(1); break;
    }
#undef OSN_TL
#undef OSN_TL2
#undef OSN_TL3
#undef OSN_TL4
#undef OSN_TL5
#undef OSN_TL6
#undef OSN_TL7
    OSN_REQUIRE(rc_attr == OSN_OK, OSN_E_HIP, "osn_spconv_fwd_tl: cannot reserve %zu bytes of LDS for the output tile", tile_bytes);
    OSN_LAUNCH_CHECK();
    if (nz > 1) {
        const int64_t total4 = n_out * (cout / 4);
        int g = int(cdiv(total4, 256));
        if (g > 4096) g = 4096;
        hipLaunchKernelGGL(epi.mean ? tl_reduce_parts_kernel<true> : tl_reduce_parts_kernel<false>, dim3(g), dim3(256), 0, st,
                           reinterpret_cast<const float4*>(partial), nz, n_out, cout / 4, out_rows, reinterpret_cast<float4*>(out), epi);
        OSN_LAUNCH_CHECK();
    }
    return OSN_OK;
}

int osn::spconv_fwd_tl_epi(const float* in, int64_t n_in, const void* Wp, const void* tl, const int32_t* out_rows, float* out,
                           int64_t n_out, int K, int cin, int cout, int bm, void* ws, size_t ws_bytes, int32_t* counters, const Epi& epi,
                           osn_stream_t stream, int pieces) {
    OSN_REQUIRE(counters, OSN_E_ARG, "spconv_fwd_tl_epi: null counters");
    return spconv_fwd_tl_impl(in, n_in, Wp, tl, out_rows, out, nullptr, n_out, K, cin, cout, bm, ws, ws_bytes, counters, nullptr, stream, epi,
                              pieces);
}

extern "C" int osn_spconv_fwd_tl(const float* in, int64_t n_in, const void* Wp, const void* tl, const int32_t* out_rows,
                                 float* out, double* bn_partial, int64_t n_out, int K, int cin, int cout, int bm, void* ws,
                                 size_t ws_bytes, int32_t* counters, osn_stream_t stream) {
    return spconv_fwd_tl_impl(in, n_in, Wp, tl, out_rows, out, bn_partial, n_out, K, cin, cout, bm, ws, ws_bytes, counters, nullptr,
                              stream, epi_none(), 3);
}

extern "C" int osn_spconv_fwd_tl_pieces(const float* in, int64_t n_in, const void* Wp, const void* tl, const int32_t* out_rows,
                                        float* out, double* bn_partial, int64_t n_out, int K, int cin, int cout, int bm, void* ws,
                                        size_t ws_bytes, int32_t* counters, osn_stream_t stream, int pieces) {
    return spconv_fwd_tl_impl(in, n_in, Wp, tl, out_rows, out, bn_partial, n_out, K, cin, cout, bm, ws, ws_bytes, counters, nullptr,
                              stream, epi_none(), pieces);
}

// Tools only (not part of include/openscene_amd.h, NOT in the product library: built with OSN_BUILD_TOOLS=1 python -m openscene_amd.build):
// the same launch with the phase timers of wave 0 of every workgroup written to prof[512][10] (s_memtime ticks; tools/prof_tl.py).
#ifdef OSN_BUILD_TOOLS
extern "C" int osn_dbg_spconv_fwd_tl_prof(const float* in, int64_t n_in, const void* Wp, const void* tl,
                                          const int32_t* out_rows, float* out, int64_t n_out, int K, int cin, int cout,
                                          int bm, void* ws, size_t ws_bytes, long long* prof, osn_stream_t stream) {
    return spconv_fwd_tl_impl(in, n_in, Wp, tl, out_rows, out, nullptr, n_out, K, cin, cout, bm, ws, ws_bytes, nullptr, prof, stream);
}
#endif
