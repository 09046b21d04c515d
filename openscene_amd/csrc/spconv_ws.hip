// Sparse 3-D convolution on gfx950 for the SMALL maps (<= 16 k rows): weight-stationary workgroups over the per-offset
// pair arrays, partial rows per offset, ordered sum.
//
// Function parity (not a port) with MinkowskiEngine's convolution kernels:
//   out[o] = sum_k in[nbr[k,o]] @ W[k]      (forward, and -- on the transposed map with the mirrored / transposed weight
//                                            image -- the input gradient).
//
// Why another kernel (measured): on the 13 k / 3.3 k / 730-row levels of a 100 k-voxel
// scene an output-stationary tile (spconv_fwd_x6, spconv_tl) meets a (tile, offset) with 10-30 real pairs and has to
// bring the offset's WHOLE weight slice (128 x 128 x 3 bf16 planes = 98 KB) into the CU for it: 52-210 tiles x 27 offsets
// x 98 KB = 140-560 MB through the 64 B/clk load path of the CUs for a convolution of 0.04-0.2 M pairs -- 45-100 us each
// at 25-50 TF, with a per-workgroup chain of 27 fragment loads.  Here the roles are swapped:
//   * a workgroup owns ONE offset k and a chunk of <= 128 of its pairs (pin / pout / poff of osn_pair_lists_build, the
//     arrays the weight gradient already uses): W[k]'s B fragments are loaded once into registers and multiply every
//     pair of the chunk -- weight traffic drops to (chunks x 98 KB), the chain to one fragment load + <= 4 steps;
//   * the result row of pair (i -> o) at offset k goes to partial[k][o] (a row is written by exactly one workgroup:
//     an output row has at most one input row per offset);
//   * a second kernel sums out[o] = sum over k ascending of partial[k][o] for the offsets the map has at o (the
//     neighbour table of the destination side tells which) => fixed summation order, bitwise reproducible.
// The partial rows cost pairs x Cout x 4 B written and read once (20-150 MB on these levels, L2 / Infinity-Cache
// resident), which is why the 48 k / 100 k-row levels stay on the tile-list kernel.
// Arithmetic: "bf16x6" as in spconv_tl.hip (three bf16 pieces per operand, six MFMAs per product block, fp32 accumulate).
#include "common.h"
#include "split.h"
#include "pairlist.h"
#include "epilogue.h"

namespace osn {

constexpr int WS_NG = 4;            // 32-pair steps per workgroup at most
constexpr int WS_CH = 32 * WS_NG;   // pairs per workgroup at most

// 4 waves; wave w < NW owns output columns [32 w, 32 w + 32) of the workgroup's column group (waves >= NW only gather
// and stage); KS k-steps of 32 input channels per chunk (B fragments of a chunk: KS x 2 column blocks x 3 planes).
// EPI (inference, direct launches): the stage's evaluation-mode batch norm in the epilogue (epilogue.h)
// The kernel's text is spconv_ws_kernel.h, included once per kernel template; per accumulator its products and their order are those of
// split_products() in split.h, for the template's piece count.
// the three-piece kernel, under the name and template parameters it always had ...
#define OSN_WS_TEMPLATE template <int NW, int KS, bool EPI = false>
#define OSN_WS_NAME spconv_ws_kernel
#define OSN_WS_NP 3
#include "spconv_ws_kernel.h"
#undef OSN_WS_TEMPLATE
#undef OSN_WS_NAME
#undef OSN_WS_NP
// ... and the reduced inference modes: the same text with NP_ = 2 or 1 pieces
#define OSN_WS_TEMPLATE template <int NP_, int NW, int KS, bool EPI = false>
#define OSN_WS_NAME spconv_ws_pieces_kernel
#define OSN_WS_NP NP_
#include "spconv_ws_kernel.h"
#undef OSN_WS_TEMPLATE
#undef OSN_WS_NAME
#undef OSN_WS_NP

// out[r] = sum over k ascending, nbr[k][r] >= 0, of partial[k][r]  (rows without any neighbour: zeros)
// KT: offsets of the map when it is one of the two sizes the U-Net has (loads in flight in groups of WS_RED_GROUP), else 0.
// At most 64 VGPRs (8 waves per SIMD): the reductions of the backward pass run beside the weight gradients and get the registers
// those leave.
constexpr int WS_RED_GROUP = 9;
template <int KT, bool EPI = false>
__global__ __launch_bounds__(256, 8) void spconv_ws_reduce_kernel(const float* __restrict__ partial, const int32_t* __restrict__ nbr,
                                                               const float* __restrict__ zeros, float* __restrict__ out,
                                                               int64_t n_dst, int K, int c4, const Epi epi) {
    const int64_t total = n_dst * c4;
    const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int64_t r = e / c4;
    const int c = int(e - r * c4);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (KT > 0) {
        // unconditional loads (an absent offset reads a line of zeros: x + 0 == x), WS_RED_GROUP independent quads per thread at a
        // time and the adds in ascending k behind each group: s = ((0 + v0) + v1) + ..., the sum all K quads in flight gave, bit for
        // bit, with 36 registers of quads instead of 4 K (108 at K = 27: no wave of this kernel fitted beside a weight-gradient
        // launch).  The K table entries are read first, all at once, into one mask: a group is one round trip.
        constexpr int G = KT > 0 && KT % WS_RED_GROUP == 0 ? WS_RED_GROUP : (KT > 0 ? KT : 1);
        static_assert(KT <= 32 && (KT <= 0 || KT % G == 0), "one mask word, whole groups");
        unsigned present = 0;
#pragma unroll
        for (int k = 0; k < KT; ++k) present |= (nbr[int64_t(k) * n_dst + r] >= 0 ? 1u : 0u) << k;
#pragma unroll 1
        for (int k0 = 0; k0 < KT; k0 += G) {                 // (a loop, not unrolled: unrolled, all K loads are hoisted to the top again)
            float4 v[G];
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const float* src = (present >> (k0 + j)) & 1u ? partial + ((int64_t(k0 + j) * n_dst + r) * c4 + c) * 4 : zeros;
                v[j] = *reinterpret_cast<const float4*>(src);
            }
#pragma unroll
            for (int j = 0; j < G; ++j) { s.x += v[j].x; s.y += v[j].y; s.z += v[j].z; s.w += v[j].w; }
        }
    } else {
        for (int k = 0; k < K; ++k) {
            if (nbr[int64_t(k) * n_dst + r] >= 0) {
                const float4 v = *reinterpret_cast<const float4*>(partial + ((int64_t(k) * n_dst + r) * c4 + c) * 4);
                s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            }
        }
    }
    if constexpr (EPI) s = epi_quad(epi, s, r, 4 * c, 4 * c4);                 // evaluation-mode batch norm (epilogue.h)
    reinterpret_cast<float4*>(out)[e] = s;
}

static int ws_waves(int cout) {
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

// 256 bytes of zeros + the partial rows [K][n_dst][cout]
extern "C" size_t osn_spconv_fwd_ws_ws_bytes(int64_t n_dst, int K, int cout, int direct) {
    return 256 + (direct ? 0 : size_t(K) * size_t(n_dst > 0 ? n_dst : 0) * size_t(cout) * 4);
}

int osn::spconv_fwd_ws_epi(const float* in, int64_t n_in, const void* Wp, const void* pl, int64_t pl_rows, int swap, int direct,
                           const int32_t* nbr_dst, float* out, int64_t n_dst, int K, int cin, int cout, void* ws, size_t ws_bytes,
                           const Epi& epi, osn_stream_t stream, int pieces) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(pieces >= 1 && pieces <= 3, OSN_E_ARG, "osn_spconv_fwd_ws: pieces=%d (1, 2 or 3)", pieces);
    OSN_REQUIRE(n_dst >= 0 && n_dst < (int64_t(1) << 31) && n_in >= 0 && n_in < (int64_t(1) << 31), OSN_E_ARG,
                "osn_spconv_fwd_ws: row counts out of range");
    OSN_REQUIRE(K >= 2 && K <= PL_KMAX && cin >= 4 && (cin & 3) == 0 && cout >= 4 && (cout & 3) == 0, OSN_E_ARG,
                "osn_spconv_fwd_ws: needs 2 <= K <= %d, cin %% 4 == 0, cout %% 4 == 0 (K=%d cin=%d cout=%d)", PL_KMAX, K, cin, cout);
    OSN_REQUIRE(pl_rows == (swap ? n_in : n_dst), OSN_E_ARG,
                "osn_spconv_fwd_ws: the pair arrays are of a map with %lld output rows, this launch writes %lld rows (swap=%d)",
                (long long)pl_rows, (long long)(swap ? n_in : n_dst), swap);
    if (n_dst == 0) return OSN_OK;
    OSN_REQUIRE(in && Wp && pl && (nbr_dst || direct) && out, OSN_E_ARG, "osn_spconv_fwd_ws: null pointer");
    OSN_REQUIRE(aligned16(in) && aligned16(Wp) && aligned16(out) && aligned16(ws), OSN_E_ARG, "osn_spconv_fwd_ws: pointers must be 16-byte aligned");
    const size_t need = osn_spconv_fwd_ws_ws_bytes(n_dst, K, cout, direct);
    OSN_REQUIRE(ws && ws_bytes >= need, OSN_E_WS, "osn_spconv_fwd_ws: workspace %zu < %zu", ws_bytes, need);
    PlView v = pl_view(const_cast<void*>(pl), pl_rows, K, 1);      // (the tile height only places the scratch behind the arrays)
    const int32_t* gsrc = swap ? v.pout : v.pin;
    const int32_t* gdst = swap ? v.pin : v.pout;
    float* zeros = static_cast<float*>(ws);
    float* partial = reinterpret_cast<float*>(static_cast<char*>(ws) + 256);
    const int nw = ws_waves(cout);
    const int gz = int(cdiv(cout, 32 * nw));
    const int ns = (cin + 31) / 32, ncb = (cout + 15) / 16;
    const int ks = ns <= 4 ? ns : (ns % 4 == 0 ? 4 : (ns % 3 == 0 ? 3 : 4));
    // pairs per workgroup: 64 on the deepest maps (more workgroups than CUs matters more than weight traffic), else 128;
    // an offset has at most min(n_in, n_dst) pairs
    const int64_t pmax = n_in < n_dst ? n_in : n_dst;
    const int chunk = pmax <= 4096 ? 64 : WS_CH;       // (32 / 64 / 128 measured within 5 % of each other)
    const dim3 grid(unsigned(cdiv(pmax, chunk)), unsigned(K), unsigned(gz));
    const bf16x8* wp = static_cast<const bf16x8*>(Wp);
#define OSN_WS3(KERN_E_, KERN_)                                                                                        \
    do {                                                                                                               \
        if (direct && epi.mean)                                                                                        \
            hipLaunchKernelGGL((KERN_E_), grid, dim3(256), 0, st, in, wp, gsrc, gdst, v.poff, out, zeros,              \
                               int(n_dst), K, cin, cout, ns, ncb, chunk, direct, epi);                                 \
        else                                                                                                           \
            hipLaunchKernelGGL((KERN_), grid, dim3(256), 0, st, in, wp, gsrc, gdst, v.poff,                            \
                               direct ? out : partial, zeros, int(n_dst), K, cin, cout, ns, ncb, chunk, direct, epi_none()); \
    } while (0)
#define OSN_WS2(NW_, KS_)                                                                                              \
    do {                                                                                                               \
        if (pieces == 3) OSN_WS3((spconv_ws_kernel<NW_, KS_, true>), (spconv_ws_kernel<NW_, KS_, false>));             \
        else if (pieces == 2) OSN_WS3((spconv_ws_pieces_kernel<2, NW_, KS_, true>), (spconv_ws_pieces_kernel<2, NW_, KS_, false>)); \
        else OSN_WS3((spconv_ws_pieces_kernel<1, NW_, KS_, true>), (spconv_ws_pieces_kernel<1, NW_, KS_, false>));     \
    } while (0)
#define OSN_WS(NW_)                                                                                                    \
    do {                                                                                                               \
        switch (ks) {                                                                                                  \
            case 1: OSN_WS2(NW_, 1); break;                                                                            \
            case 2: OSN_WS2(NW_, 2); break;                                                                            \
            case 3: OSN_WS2(NW_, 3); break;                                                                            \
            default: OSN_WS2(NW_, 4); break;                                                                           \
        }                                                                                                              \
    } while (0)
    switch (nw) {
        case 4: OSN_WS(4); break;
        case 3: OSN_WS(3); break;
        case 2: OSN_WS(2); break;
        default: OSN_WS(1); break;
    }
#undef OSN_WS
#undef OSN_WS2
#undef OSN_WS3
    if (direct) {
        OSN_LAUNCH_CHECK();
        return OSN_OK;
    }
    const int c4 = cout / 4;
    const dim3 rgrid(unsigned(cdiv(n_dst * c4, 256)));
#define OSN_WSR(KT_)                                                                                                                    \
    do {                                                                                                                                \
        if (epi.mean) hipLaunchKernelGGL((spconv_ws_reduce_kernel<KT_, true>), rgrid, dim3(256), 0, st, partial, nbr_dst, zeros, out, n_dst, K, c4, epi); \
        else hipLaunchKernelGGL((spconv_ws_reduce_kernel<KT_, false>), rgrid, dim3(256), 0, st, partial, nbr_dst, zeros, out, n_dst, K, c4, epi);         \
    } while (0)
    if (K == 27) OSN_WSR(27);
    else if (K == 8) OSN_WSR(8);
    else OSN_WSR(0);
#undef OSN_WSR
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_spconv_fwd_ws(const float* in, int64_t n_in, const void* Wp, const void* pl, int64_t pl_rows,
                                 int swap, int direct, const int32_t* nbr_dst, float* out, int64_t n_dst, int K, int cin, int cout,
                                 void* ws, size_t ws_bytes, osn_stream_t stream) {
    return spconv_fwd_ws_epi(in, n_in, Wp, pl, pl_rows, swap, direct, nbr_dst, out, n_dst, K, cin, cout, ws, ws_bytes, epi_none(), stream, 3);
}

extern "C" int osn_spconv_fwd_ws_pieces(const float* in, int64_t n_in, const void* Wp, const void* pl, int64_t pl_rows,
                                        int swap, int direct, const int32_t* nbr_dst, float* out, int64_t n_dst, int K, int cin, int cout,
                                        void* ws, size_t ws_bytes, osn_stream_t stream, int pieces) {
    return spconv_fwd_ws_epi(in, n_in, Wp, pl, pl_rows, swap, direct, nbr_dst, out, n_dst, K, cin, cout, ws, ws_bytes, epi_none(), stream,
                             pieces);
}
