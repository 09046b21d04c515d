// Sparse 3-D convolution on gfx950 for NARROW layers (32 / 64 channels): register gather, no LDS staging, no barrier in the loop.
//
// Function parity (not a port) with MinkowskiEngine's convolution kernels:
//   out[o] = sum_k in[nbr[k, o]] @ W[k]        (forward; with the input-gradient weight image and the mirrored table: the input gradient)
// for the convolutions the other kernels serve badly (round 5's per-stage table, profiles/r05_s20_bench_detail.json): the 32 -> 32
// 3^3 layers of the 52 k-row level and the 32 / 64-channel layers of the 13 k-row level ran 30 - 50 us each on the first-generation
// kernel (spconv.hip: 128-row tiles, gathered rows AND the weight chunk staged through LDS, two barriers per (offset, chunk)) for
// 1 - 3 us of matrix work -- a chain of ~30 barrier-separated stages per tile.  With <= 64 input channels none of that machinery is
// needed:
//   * the A operand of v_mfma_f32_16x16x32_bf16 is "lane l: row l & 15, 8 consecutive channels 8 (l >> 4) ..": exactly 32 bytes of
//     one gathered fp32 row.  Every lane loads ITS 32 bytes straight from the feature matrix (two 16-byte buffer loads through the
//     neighbour table; an absent neighbour is an out-of-range offset: the load returns zeros and moves no data), splits them into the
//     three bf16 pieces in registers and multiplies -- no staging buffer, no LDS round trip, no barrier;
//   * the weight fragments of one offset (<= 24 KB) are loaded once per offset and wave from the fragment-order image the tile-list
//     kernel uses (osn_weight_prep_tl), and reused over all row blocks of the workgroup;
//   * a workgroup = 64 (x HALVES) table rows; its four waves take the offsets k = w, w + 4, ... (a quarter of the chain each) and
//     their partial tiles are summed through LDS in wave order at the end => fixed summation order, bitwise reproducible;
//   * (block, offset) groups without a single pair skip their MFMAs (wave-uniform); on a tile-ordered table (osn_kmap_sort) most are.
// Arithmetic: "bf16x6" as everywhere (split.h: three bf16 pieces per operand, six MFMAs per product block, fp32 accumulate).
#include "common.h"
#include "split.h"
#include "epilogue.h"

namespace osn {

constexpr int RG_RB = 4;                 // 16-row blocks per wave and half: 64 rows

// KS = input channels / 32 (1, 2), NCB = output channels / 16 (2, 4), HALVES = 64-row halves per workgroup (weight fragments reused)
// OCC: workgroups per CU the register allocation is held to (32 -> 32: 168 registers without a spill = three workgroups per CU, all
// 745 workgroups of the 48 k-row level resident at once; the 64-channel instances need more)
// BD: the weight fragments of the NEXT offset loaded one iteration ahead into a second register set.  Measured SLOWER (48 k rows
// 32 -> 32: 24.8 against 22.0 us; 13 k rows 32 -> 64: 18.9 / 15.6): the extra registers cost a resident workgroup per CU, and resident
// waves are what hides this kernel's per-offset latency chain.  Not instantiated.
// EPI (inference): the stage's evaluation-mode batch norm in the epilogue (epilogue.h)
// The kernel's text is spconv_rg_kernel.h, included once per kernel template; per accumulator its products and their order are those of
// split_products() in split.h, for the template's piece count.
// the three-piece kernel, under the name and template parameters it always had ...
#define OSN_RG_TEMPLATE template <int KS, int NCB, int HALVES, int OCC, bool BD, bool EPI = false>
#define OSN_RG_NAME spconv_rg_kernel
#define OSN_RG_NP 3
#include "spconv_rg_kernel.h"
#undef OSN_RG_TEMPLATE
#undef OSN_RG_NAME
#undef OSN_RG_NP
// ... and the reduced inference modes: the same text with NP_ = 2 or 1 pieces (OCC as the three-piece instance of the shape: a reduced
// instance needs fewer registers and is held to no less)
#define OSN_RG_TEMPLATE template <int NP_, int KS, int NCB, int HALVES, int OCC, bool BD, bool EPI = false>
#define OSN_RG_NAME spconv_rg_pieces_kernel
#define OSN_RG_NP NP_
#include "spconv_rg_kernel.h"
#undef OSN_RG_TEMPLATE
#undef OSN_RG_NAME
#undef OSN_RG_NP

}  // namespace osn

using namespace osn;

// shapes the kernel takes: 32 or 64 channels on both sides, a table (K > 1), a feature matrix below 2 GB and 2^24 rows
extern "C" int osn_spconv_fwd_rg_ok(int64_t n_in, int K, int cin, int cout) {
    return K > 1 && K <= 128 && (cin == 32 || cin == 64) && (cout == 32 || cout == 64) && n_in >= 1 && n_in < (int64_t(1) << 24) &&
           uint64_t(n_in) * uint64_t(cin) * 4u < (uint64_t(1) << 31);
}

int osn::spconv_fwd_rg_epi(const float* in, int64_t n_in, const void* Wp, const int32_t* nbr, const int32_t* out_rows, float* out,
                           int64_t n_out, int K, int cin, int cout, const Epi& epi, osn_stream_t stream, int pieces) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(pieces >= 1 && pieces <= 3, OSN_E_ARG, "osn_spconv_fwd_rg: pieces=%d (1, 2 or 3)", pieces);
    OSN_REQUIRE(n_out >= 0 && n_out < (int64_t(1) << 31), OSN_E_ARG, "osn_spconv_fwd_rg: n_out out of range");
    OSN_REQUIRE(osn_spconv_fwd_rg_ok(n_in > 0 ? n_in : 1, K, cin, cout), OSN_E_ARG,
                "osn_spconv_fwd_rg: needs K > 1, 32 or 64 channels on both sides, a feature matrix below 2 GB (K=%d cin=%d cout=%d n_in=%lld)",
                K, cin, cout, (long long)n_in);
    if (n_out == 0) return OSN_OK;
    OSN_REQUIRE(in && Wp && nbr && out, OSN_E_ARG, "osn_spconv_fwd_rg: null pointer");
    OSN_REQUIRE(aligned16(in) && aligned16(Wp) && aligned16(out), OSN_E_ARG, "osn_spconv_fwd_rg: pointers must be 16-byte aligned");
    const unsigned in_bytes = unsigned(uint64_t(n_in) * uint64_t(cin) * 4u);
    const bf16x8* wp = static_cast<const bf16x8*>(Wp);
    const int ks = cin / 32, ncb = cout / 16;
    // (two 64-row halves per workgroup -- each offset's fragments loaded once for both -- need 256 + registers: not instantiated)
    const dim3 grid(unsigned(cdiv(n_out, 64)));
#define OSN_RG_L(...) hipLaunchKernelGGL((__VA_ARGS__), grid, dim3(256), 0, st, in, wp, nbr, out_rows, out, int(n_out), K, cin, cout, in_bytes, epi)
#define OSN_RG(KS_, NCB_, H_, OCC_, BD_)                                                                                                              \
    do {                                                                                                                                              \
        if (pieces == 3) {                                                                                                                            \
            if (epi.mean) OSN_RG_L(spconv_rg_kernel<KS_, NCB_, H_, OCC_, BD_, true>);                                                                 \
            else OSN_RG_L(spconv_rg_kernel<KS_, NCB_, H_, OCC_, BD_, false>);                                                                         \
        } else if (pieces == 2) {                                                                                                                     \
            if (epi.mean) OSN_RG_L(spconv_rg_pieces_kernel<2, KS_, NCB_, H_, OCC_, BD_, true>);                                                       \
            else OSN_RG_L(spconv_rg_pieces_kernel<2, KS_, NCB_, H_, OCC_, BD_, false>);                                                               \
        } else {                                                                                                                                      \
            if (epi.mean) OSN_RG_L(spconv_rg_pieces_kernel<1, KS_, NCB_, H_, OCC_, BD_, true>);                                                       \
            else OSN_RG_L(spconv_rg_pieces_kernel<1, KS_, NCB_, H_, OCC_, BD_, false>);                                                               \
        }                                                                                                                                             \
    } while (0)
    if (ks == 1 && ncb == 2) OSN_RG(1, 2, 1, 3, false);
    else if (ks == 1 && ncb == 4) OSN_RG(1, 4, 1, 2, false);
    else if (ks == 2 && ncb == 2) OSN_RG(2, 2, 1, 2, false);
    else OSN_RG(2, 4, 1, 1, false);
#undef OSN_RG
#undef OSN_RG_L
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_spconv_fwd_rg(const float* in, int64_t n_in, const void* Wp, const int32_t* nbr, const int32_t* out_rows,
                                 float* out, int64_t n_out, int K, int cin, int cout, osn_stream_t stream) {
    return spconv_fwd_rg_epi(in, n_in, Wp, nbr, out_rows, out, n_out, K, cin, cout, epi_none(), stream, 3);
}

extern "C" int osn_spconv_fwd_rg_pieces(const float* in, int64_t n_in, const void* Wp, const int32_t* nbr, const int32_t* out_rows,
                                        float* out, int64_t n_out, int K, int cin, int cout, osn_stream_t stream, int pieces) {
    return spconv_fwd_rg_epi(in, n_in, Wp, nbr, out_rows, out, n_out, K, cin, cout, epi_none(), stream, pieces);
}
