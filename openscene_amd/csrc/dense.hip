// 1x1 convolutions on gfx950: out[N, Cout] = in[N, Cin] @ B  -- the U-Net's head (`final`, 96 -> 768), the BasicBlock
// shortcut convolutions, their input gradients, and the folded head of the fused queries.
//
// Function parity (not a port) with [ME] MinkowskiConvolution(kernel_size=1) (models/mink_unet.py:108-113,
// models/resnet_base.py:101-107): a plain row-wise matrix product, no kernel map.
//
// Why a kernel of its own (measured): the gather kernels treat a 1x1 conv as a one-offset
// map -- 32-row steps with two barriers each, the result block added into an LDS tile -- and run the head at 92 TF
// (161 us), a 128 -> 96 shortcut on 100 k rows at 16 TF (153 us): 10x off either roof.  Without a map there is nothing
// to compact: a workgroup takes 64 consecutive rows, stages their split-bf16 pieces ONCE per channel chunk, and every
// wave multiplies them with the fragments of its 32 output columns held in registers -- 4 row blocks x 2 column blocks
// x 6 products per k-step between two barriers -- and stores its accumulators straight to the output rows.  When the
// whole contraction fits one chunk (Cin <= 128: the head, most shortcuts) the staged rows serve ALL column groups of the
// workgroup, so the input is read and split once.  Same arithmetic as spconv_tl.hip ("bf16x6", split.h) and the
// same weight image (osn_weight_prep_tl with K = 1).
#include "common.h"
#include "split.h"
#include "epilogue.h"

namespace osn {

constexpr int DN_BM = 64;           // rows per workgroup

// 4 waves; wave w owns output columns [128 cg + 32 w, + 32) of column group cg; KS k-steps of 32 input channels per chunk
// EPI (inference): the stage's evaluation-mode batch norm in the epilogue (epilogue.h); a template flag so that the training instances
// keep their register allocation
// The kernel's text is dense_kernel.h, included once per kernel template; per accumulator its products and their order are those of
// split_products() in split.h, for the template's piece count.
// the three-piece kernel, under the name and template parameters it always had ...
#define OSN_DN_TEMPLATE template <int KS, bool EPI = false>
#define OSN_DN_NAME dense_kernel
#define OSN_DN_NP 3
#include "dense_kernel.h"
#undef OSN_DN_TEMPLATE
#undef OSN_DN_NAME
#undef OSN_DN_NP
// ... and the reduced inference modes: the same text with NP_ = 2 or 1 pieces
#define OSN_DN_TEMPLATE template <int NP_, int KS, bool EPI = false>
#define OSN_DN_NAME dense_pieces_kernel
#define OSN_DN_NP NP_
#include "dense_kernel.h"
#undef OSN_DN_TEMPLATE
#undef OSN_DN_NAME
#undef OSN_DN_NP

}  // namespace osn

using namespace osn;

// routing limit of the 1x1 kernel; narrower than what osn_dense_fwd accepts (cin >= 4)
extern "C" int osn_dense_fwd_ok(int cin, int cout) { return cin >= 8 && (cin & 3) == 0 && cout >= 4 && (cout & 3) == 0; }

int osn::dense_fwd_epi(const float* in, const void* Wp, float* out, int64_t n, int cin, int cout, const Epi& epi, osn_stream_t stream,
                       int pieces) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    OSN_REQUIRE(pieces >= 1 && pieces <= 3, OSN_E_ARG, "osn_dense_fwd: pieces=%d (1, 2 or 3)", pieces);
    OSN_REQUIRE(n >= 0 && n < (int64_t(1) << 31) && cin >= 4 && (cin & 3) == 0 && cout >= 4 && (cout & 3) == 0, OSN_E_ARG,
                "osn_dense_fwd: needs cin %% 4 == 0 and cout %% 4 == 0 (n=%lld cin=%d cout=%d)", (long long)n, cin, cout);
    if (n == 0) return OSN_OK;
    OSN_REQUIRE(in && Wp && out && aligned16(in) && aligned16(Wp) && aligned16(out), OSN_E_ARG, "osn_dense_fwd: null or unaligned pointer");
    const int ns = (cin + 31) / 32, ncb = (cout + 15) / 16;
    const int ks = ns <= 4 ? ns : (ns % 4 == 0 ? 4 : (ns % 3 == 0 ? 3 : 4));
    const int ncg = (cout + 127) / 128;
    const int64_t per_plane = int64_t(ns) * ncb;
    const dim3 grid(unsigned(cdiv(n, DN_BM)), unsigned(ns <= ks ? 1 : ncg));
    const bf16x8* wp = static_cast<const bf16x8*>(Wp);
    switch (ks) {
#define OSN_DN_L(...) hipLaunchKernelGGL((__VA_ARGS__), grid, dim3(256), 0, st, in, wp, out, n, cin, cout, ns, ncb, per_plane, epi)
#define OSN_DN(KS_)                                                                                                              \
    do {                                                                                                                         \
        if (pieces == 3) {                                                                                                       \
            if (epi.mean) OSN_DN_L(dense_kernel<KS_, true>);                                                                     \
            else OSN_DN_L(dense_kernel<KS_, false>);                                                                             \
        } else if (pieces == 2) {                                                                                                \
            if (epi.mean) OSN_DN_L(dense_pieces_kernel<2, KS_, true>);                                                           \
            else OSN_DN_L(dense_pieces_kernel<2, KS_, false>);                                                                   \
        } else {                                                                                                                 \
            if (epi.mean) OSN_DN_L(dense_pieces_kernel<1, KS_, true>);                                                           \
            else OSN_DN_L(dense_pieces_kernel<1, KS_, false>);                                                                   \
        }                                                                                                                        \
    } while (0)
        case 1: OSN_DN(1); break;
        case 2: OSN_DN(2); break;
        case 3: OSN_DN(3); break;
        default: OSN_DN(4); break;
    }
#undef OSN_DN
#undef OSN_DN_L
    OSN_LAUNCH_CHECK();
    return OSN_OK;
}

extern "C" int osn_dense_fwd(const float* in, const void* Wp, float* out, int64_t n, int cin, int cout, osn_stream_t stream) {
    return dense_fwd_epi(in, Wp, out, n, cin, cout, epi_none(), stream, 3);
}

extern "C" int osn_dense_fwd_pieces(const float* in, const void* Wp, float* out, int64_t n, int cin, int cout, osn_stream_t stream,
                                    int pieces) {
    return dense_fwd_epi(in, Wp, out, n, cin, cout, epi_none(), stream, pieces);
}
