"""The reduced-precision convolution modes ("bf16x3": two pieces, three products; "bf16x1": one piece, one product) without a GPU.

What gives tests/test_gpu_conv_pieces.py its teeth, on every forward case of the four families (conv_pieces.FWD_CASES) and the five
operand kinds, with conv_bounds.split_emulation (fp32 accumulation, smallest products first) standing in for a kernel.  Figures of
this module's own run (distance = worst |a - b| / (2e-6 abs-sum + half ulp + floor), conv_pieces.distance):

  * the emulation meets both bounds of its mode: within FWD_C of its own target (worst 0.38 at two pieces, 0.36 at one), and within
    C2 / C1 of the exact value: worst 0.60 of C2 ("wide_elements"), 0.992 of C1 ("piece_aligned", every case: tight by construction);
    no element out of bounds;
  * a two-piece sum that LOSES "21" or "12" sits 117 x to 1882 x FWD_C from the two-piece target on "row_scales", "gradient_sized",
    "wide_elements" and "piece_aligned" (the worst element of each (case, kind): never below 117; asserted: 100).  "cancellation" shows
    a lost h2(a) h1(b) (25 x - 1812 x) but cannot show a lost h1(a) h2(b) (0.0 - 4.8 x: the weights of a cancelling channel pair are
    EQUAL, so h1(a) h2(b) cancels like the exact product does) -- the five kinds together are needed, and the GPU module runs all five;
  * the SIX-product result sits 1.4 x to 9.7 x FWD_C from the two-piece target on "wide_elements" in every case (3.1 x on "row_scales";
    0.2 x - 5.1 x on the other kinds), and 25 x or more from the one-piece target on every kind: a kernel that ignores `pieces` fails
    the first bound;
  * "piece_aligned" cannot tell six products from three (its 22 and 13 + 31 products cancel: 2^-16 - 2 * 2^-17): distance 0.1 - 0.4.

Then the host side: the `_pieces` entries and the osn_net_run flags refuse bad arguments before anything is launched (this machine's
HIP runtime has no device: a launch would fail differently), the header declares what the library exports, the kernel texts take
their plane counts from the piece count, and openscene_amd.conv_precision behaves as a context manager should.
"""
import ctypes
import os
import re

import pytest
import torch

import conv_bounds as cb
import conv_pieces as cp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_KINDS = ("row_scales", "gradient_sized", "wide_elements", "piece_aligned")


@pytest.fixture(autouse=True, scope="module")
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 8))
    yield
    torch.set_num_threads(n)


def _emulate(case, nbr, kind, keep):
    feats, w, _ = cb.operands(case, kind)
    return cb.split_emulation(feats, w, keep, nbr, case.n_in)


@pytest.mark.parametrize("case", cp.FWD_CASES, ids=cp.FWD_IDS)
def test_emulated_modes_meet_both_bounds_and_mistakes_do_not(case):
    case, nbr = cb.resolve(case)
    for kind in cb.KINDS:
        ref = cb.reference(case, kind)
        six = _emulate(case, nbr, kind, cp.KEEP[3])
        for pieces in (2, 1):
            want = cp.target(case, kind, pieces)
            got = _emulate(case, nbr, kind, cp.KEEP[pieces])
            label = "%s %s, %d pieces" % (case.id, kind, pieces)
            r_own = cb.within(got, want, ref.b_out, cb.FWD_C, label + " against its target")
            r_exact = cb.within(got, ref.out, ref.b_out, cp.C_EXACT[pieces], label + " against the exact value")
            d_six = cp.distance(six, want, ref.b_out)
            print("EMU %s %s pieces=%d own %.3f exact %.3f six-product distance %.1f" % (case.id, kind, pieces, r_own, r_exact, d_six))
            # a kernel that ignores `pieces` (computes six products): outside the first bound -- at one piece on every kind, at two
            # pieces on "wide_elements"; "piece_aligned" cannot tell six from three
            if pieces == 1:
                assert d_six >= 25.0, "%s: six products only %.1f x FWD_C from the one-piece target" % (label, d_six)
            elif kind == "wide_elements":
                assert 1.0 < d_six, "%s: six products only %.2f x FWD_C from the two-piece target" % (label, d_six)
            elif kind == "piece_aligned":
                assert d_six < 1.0, "%s: piece_aligned was not expected to tell six products from three (%.2f)" % (label, d_six)
        # a two-piece sum that loses one of its 2^-8 products
        want2 = cp.target(case, kind, 2)
        for drop in ("21", "12"):
            lost = _emulate(case, nbr, kind, [ij for ij in cp.KEEP[2] if ij != drop])
            d = cp.distance(lost, want2, ref.b_out)
            print("LOST %s %s h%sh%s distance %.1f" % (case.id, kind, drop[0], drop[1], d))
            if kind in LOSS_KINDS:
                assert d >= 100.0, "%s %s: a lost h%sh%s sits only %.1f x FWD_C from the two-piece target" % (case.id, kind, drop[0], drop[1], d)


def test_keep_lists_follow_the_rule_and_the_constants_their_derivation():
    for p in (1, 2, 3):
        assert [ij for ij in cp.KEEP[p]] == sorted(cp.KEEP[p], key=lambda ij: -(int(ij[0]) + int(ij[1])))       # smallest first
        assert all(int(ij[0]) + int(ij[1]) <= p + 1 for ij in cp.KEEP[p]) and len(cp.KEEP[p]) == p * (p + 1) // 2
    assert cp.C_EXACT[2] == 2.0 ** -16 + 2 * 2.0 ** -17 + cb.FWD_C and cp.C_EXACT[1] == 2 * 2.0 ** -8 + cb.FWD_C
    assert cp.C_EXACT[3] == cb.FWD_C
    # the first pieces of an operand do not depend on how many are formed: a reduced launch reads a prefix of the same image
    x = cb.adversarial("wide_elements", 64, 8, torch.Generator().manual_seed(1))
    assert torch.equal(cb.split3(x)[0], x.bfloat16().float())


# ------------------------------------------------------------------------------------------------------------ the C ABI
NEW_ENTRIES = {"osn_spconv_fwd_tl_pieces": "osn_spconv_fwd_tl", "osn_spconv_fwd_rg_pieces": "osn_spconv_fwd_rg",
               "osn_spconv_fwd_ws_pieces": "osn_spconv_fwd_ws", "osn_dense_fwd_pieces": "osn_dense_fwd"}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from openscene_amd import _lib
    return _lib.load()


def test_header_declares_the_new_entries_next_to_their_contract(lib):
    from openscene_amd import _lib
    src = open(os.path.join(ROOT, "include", "openscene_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, base in NEW_ENTRIES.items():
        assert hasattr(lib, name), name
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code, flags=re.S).group(1)
        base_decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % base, code, flags=re.S).group(1)
        norm = lambda t: [re.sub(r"\s+", " ", a).strip() for a in t.split(",")]
        assert norm(decl) == norm(base_decl) + ["int pieces"], name                  # the base entry's arguments + a trailing `int pieces`
        assert _lib.PROTOTYPES[name] == (_lib.PROTOTYPES[base][0], _lib.PROTOTYPES[base][1] + [ctypes.c_int]), name
    block = src[src.index("reduced-precision inference"):src.index("int osn_spconv_fwd_tl_pieces(")]
    for word in ("31 22 13 21 12 11", "21 12 11", "i + j <= pieces + 1", "planes 0 .. pieces - 1", "2^-15 + 2e-6", "2^-7 + 2e-6",
                 "OSN_E_ARG", "run/evaluate.py:290-292", "models/mink_unet.py:47-113", "six-product kernel"):
        assert word in block, word
    assert re.search(r"#define\s+OSN_NET_RUN_PIECES_2\s+4\b", src) and re.search(r"#define\s+OSN_NET_RUN_PIECES_1\s+8\b", src)
    assert lib.osn_version() == 3


def test_pieces_out_of_range_is_refused_before_anything_else(lib):
    from openscene_amd import _lib
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 15) & ~15
    for bad in (0, 4, -1):
        calls = {
            "osn_dense_fwd": lambda: lib.osn_dense_fwd_pieces(p, p, p, 8, 16, 16, None, bad),
            "osn_spconv_fwd_rg": lambda: lib.osn_spconv_fwd_rg_pieces(p, 8, p, p, None, p, 8, 27, 32, 32, None, bad),
            "osn_spconv_fwd_ws": lambda: lib.osn_spconv_fwd_ws_pieces(p, 8, p, p, 8, 0, 0, p, p, 8, 27, 32, 32, p, 4096, None, bad),
            "osn_spconv_fwd_tl": lambda: lib.osn_spconv_fwd_tl_pieces(p, 8, p, p, None, p, None, 8, 27, 32, 32, 32, p, 4096, None, None, bad),
        }
        for name, call in calls.items():
            assert call() == -1, (name, bad)                               # OSN_E_ARG
            assert _lib.last_error().startswith("%s: pieces=%d" % (name, bad)), _lib.last_error()
    # a valid piece count goes on to the entry's own checks (here: empty problems return OSN_OK without a launch)
    for ok in (1, 2, 3):
        assert lib.osn_dense_fwd_pieces(p, p, p, 0, 16, 16, None, ok) == 0
        assert lib.osn_spconv_fwd_rg_pieces(p, 8, p, p, None, p, 0, 27, 32, 32, None, ok) == 0
        assert lib.osn_spconv_fwd_ws_pieces(p, 8, p, p, 0, 0, 0, p, p, 0, 27, 32, 32, p, 4096, None, ok) == 0
        assert lib.osn_spconv_fwd_tl_pieces(p, 8, p, p, None, p, None, 0, 27, 32, 32, 32, p, 4096, None, None, ok) == 0


def test_net_run_flags_are_checked_before_the_first_launch(lib):
    from openscene_amd import _lib, executor as E
    assert E.RUN_PIECES == {3: 0, 2: 4, 1: 8}
    desc = E._Desc()                                   # all zero: any call that gets past the flag check fails on the descriptor

    def call(fn, flags, training):
        run = E._Run()
        run.flags, run.training = flags, training
        rc = fn(ctypes.addressof(desc), ctypes.addressof(run), None)
        return rc, _lib.last_error()

    for flags, training in ((4 | 8, 0), (4, 1), (8, 1), (4 | 8 | 2, 0), (4 | 2, 1)):
        rc, msg = call(lib.osn_net_forward, flags, training)
        assert rc == -1 and msg.startswith("osn_net_forward: flags %d" % flags), (flags, training, msg)
    for flags in (4, 8, 12, 4 | 1):
        rc, msg = call(lib.osn_net_backward, flags, 1)
        assert rc == -1 and msg.startswith("osn_net_backward: flags %d" % flags), (flags, msg)
    for fn, flags, training in ((lib.osn_net_forward, 4, 0), (lib.osn_net_forward, 8 | 2, 0), (lib.osn_net_forward, 0, 1),
                                (lib.osn_net_backward, 1, 1)):
        rc, msg = call(fn, flags, training)
        assert rc == -1 and "flags" not in msg, (flags, training, msg)         # past the flag check: the zero descriptor is what fails


def test_kernel_texts_take_their_plane_counts_from_the_piece_count():
    csrc = os.path.join(ROOT, "openscene_amd", "csrc")
    for fam in ("spconv_tl", "spconv_ws", "spconv_rg", "dense"):
        text = open(os.path.join(csrc, fam + "_kernel.h")).read()
        code = re.sub(r"//[^\n]*", "", text)
        assert "split_products<NP>(" in code and "split_products(" not in code, fam
        assert not re.search(r"\]\[3\];|pl < 3\b|stage\[3\]|\bp3\b", code), fam     # no plane count or plane loop written as a literal
        assert re.search(r"\[NP\]", code), fam
        hip = open(os.path.join(csrc, fam + ".hip")).read()
        assert hip.count('#include "%s_kernel.h"' % fam) == 2, fam             # the three-piece kernel and the reduced template
    split = open(os.path.join(csrc, "split.h")).read()
    for form in ("template <int NP>\n__device__ __forceinline__ void split1(", "template <int NP>\n__device__ __forceinline__ void tl_split4(",
                 "template <int NP>\n__device__ __forceinline__ void split8(", "template <int NP = 3, class F>"):
        assert form in split, form


# ------------------------------------------------------------------------------------------------------------ the mode selector
def test_conv_precision_semantics():
    import openscene_amd as osn
    from openscene_amd import precision
    assert precision.MODES == {v: k for k, v in cp.MODES.items()}
    base = osn.get_conv_precision()
    try:
        assert osn.set_conv_precision("bf16x6") == base
        assert precision.inference_pieces(False, False) == 3
        with osn.conv_precision("bf16x3"):
            assert osn.get_conv_precision() == "bf16x3" and precision.inference_pieces(False, False) == 2
            assert precision.inference_pieces(True, False) == 3 and precision.inference_pieces(False, True) == 3      # ignored
            with osn.conv_precision("bf16x1"):
                assert precision.inference_pieces(False, False) == 1
                with osn.conv_precision("bf16x6"):
                    assert precision.inference_pieces(False, False) == 3
                assert osn.get_conv_precision() == "bf16x1"
            assert osn.get_conv_precision() == "bf16x3"
        assert osn.get_conv_precision() == "bf16x6"
        with pytest.raises(RuntimeError):
            with osn.conv_precision("bf16x1"):
                raise RuntimeError("body")
        assert osn.get_conv_precision() == "bf16x6"                              # restored on an exception
        for bad in ("bf16x2", "fp16", "", None, 3):
            with pytest.raises(ValueError):
                osn.conv_precision(bad)
            with pytest.raises(ValueError):
                osn.set_conv_precision(bad)
        assert osn.get_conv_precision() == "bf16x6"
        # the process default, and a context over it; another thread sees the default, not this thread's context
        assert osn.set_conv_precision("bf16x1") == "bf16x6" and precision.inference_pieces(False, False) == 1
        with osn.conv_precision("bf16x3"):
            import threading
            seen = []
            t = threading.Thread(target=lambda: seen.append(osn.get_conv_precision()))
            t.start()
            t.join()
            assert seen == ["bf16x1"] and osn.get_conv_precision() == "bf16x3"
        assert osn.get_conv_precision() == "bf16x1"
    finally:
        osn.set_conv_precision(base)
    # the initial default: OSN_INFER_PRECISION, read by Python
    assert precision._initial({}) == "bf16x6" and precision._initial({"OSN_INFER_PRECISION": ""}) == "bf16x6"
    assert precision._initial({"OSN_INFER_PRECISION": "bf16x3"}) == "bf16x3"
    with pytest.raises(ValueError):
        precision._initial({"OSN_INFER_PRECISION": "fast"})


def test_wrappers_check_pieces_on_the_host():
    from openscene_amd import ops
    for bad in (0, 4, None, 2.5):
        with pytest.raises(ValueError):
            ops._pieces_ok(bad)
    assert [ops._pieces_ok(p) for p in (1, 2, 3)] == [1, 2, 3]
    import inspect
    for f in (ops.spconv_fwd_tl, ops.spconv_fwd_rg, ops.spconv_fwd_ws, ops.dense_fwd):
        assert inspect.signature(f).parameters["pieces"].default == 3, f.__name__
