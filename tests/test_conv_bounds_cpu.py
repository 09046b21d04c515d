"""What gives tests/test_gpu_conv_bounds.py its teeth, checked without a GPU: on every shape and operand kind the GPU module uses, the
CPU restatement of the split-bf16 contract (conv_bounds.split_emulation: three bf16 pieces per operand, six cross products, fp32
accumulation) meets the per-element abs-sum bound; with any ONE of the six products removed it violates the bound on the
"piece_aligned" operands, in every element that has a term; with the three discarded products added nothing moves beyond the bound.

Weight gradient: one lost product is at most 2^-16 of the abs-sum, below the weight gradient's 2e-5 = 2^-15.6 for ANY operands, so at
2e-5 only the two 2^-8 products (h1h2, h2h1) can be told apart.  The other four are separated at conv_bounds.PIECE_WGRAD_C = 2e-6,
the constant the GPU module holds the weight gradients to on "piece_aligned"; that the full emulation meets it is asserted here.

Stem, small maps (exact fp32 products, one fmaf chain in ascending offset order): the chain itself, run here in numpy, against
2e-6 * abs-sum.  Measured worst err / lim of the chain per case and kind (forward | weight gradient):
    K = 125, cin = 3, 1000 rows:  row_scales 0.21 | 0.02, cancellation 0.08 | 0.01, gradient_sized 0.12 | 0.01, wide_elements 0.27 | 0.02,
                                  piece_aligned 0.25 | 0.02
    K = 27,  cin = 4, 1000 rows:  row_scales 0.23 | 0.02, cancellation 0.01 | 0.01, gradient_sized 0.10 | 0.00, wide_elements 0.18 | 0.02,
                                  piece_aligned 0.26 | 0.01
    K = 125, cin = 3, 4100 rows:  row_scales 0.27, cancellation 0.08, gradient_sized 0.11, wide_elements 0.26, piece_aligned 0.31  (forward)
    K = 27,  cin = 4, 4100 rows:  row_scales 0.24, cancellation 0.01, gradient_sized 0.13, wide_elements 0.24, piece_aligned 0.22  (forward)
(forward against 2e-6, weight gradient against 2e-5 of the abs-sum.)  No kind exceeds the project's constants, so the stem's fp32 kernels are held to 2e-6 / 2e-5 like every other family
(STEM_FP32_BOUNDS stays empty)."""
import pytest
import torch

import conv_bounds as cb

# (case id, kind) -> bound constant taken from the CPU chain (2 x its measured worst ratio x the project's constant) where the
# chain itself exceeds the project's constant; empty: it never does (figures in the module docstring)
STEM_FP32_BOUNDS = {}


@pytest.fixture(autouse=True, scope="module")
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 8))
    yield
    torch.set_num_threads(n)


def _c_of(case):
    return cb.WGRAD_C if case.op == "wgrad" else cb.FWD_C


def _emulate(case, nbr, kind, keep):
    feats, w, gout = cb.operands(case, kind)
    if case.op == "wgrad":
        return cb.split_emulation(feats, gout, keep, nbr, case.n_in, wgrad=True)
    return cb.split_emulation(feats, w, keep, nbr, case.n_in)


def _want(case, kind):
    ref = cb.reference(case, kind)
    return (ref.gw, ref.b_gw) if case.op == "wgrad" else (ref.out, ref.b_out)


SPLIT_CASES = [c for c in cb.CASES if c.family != "stem_fp32" and not c.opt.get("perm")]


@pytest.mark.parametrize("case", SPLIT_CASES, ids=[c.id for c in SPLIT_CASES])
def test_six_products_meet_the_bound_and_each_one_is_needed(case):
    case, nbr = cb.resolve(case)
    for kind in cb.KINDS:
        want, bound = _want(case, kind)
        full = _emulate(case, nbr, kind, cb.KEPT)
        r = cb.within(full, want, bound, _c_of(case), "%s %s, six products" % (case.id, kind))
        print("emulation %s %s: worst ratio %.3f" % (case.id, kind, r))
    kind = "piece_aligned"
    want, bound = _want(case, kind)
    has_term = bound > 0
    assert int(has_term.sum()) > 0
    c_piece = cb.PIECE_WGRAD_C if case.op == "wgrad" else cb.FWD_C
    cb.within(full, want, bound, c_piece, "%s %s, six products at the piece bound" % (case.id, kind))
    for drop in cb.KEPT:
        got = _emulate(case, nbr, kind, [p for p in cb.KEPT if p != drop])
        err = (got.double() - want).abs()
        lim = c_piece * bound + 6e-8 * want.abs() + 1e-37
        assert bool((err > lim)[has_term].all()), "%s: losing h%sh%s stays inside the bound in %d elements" % (
            case.id, drop[0], drop[1], int((err <= lim)[has_term].sum()))
        if case.op == "wgrad" and drop in ("12", "21"):      # the products the weight gradient's own 2e-5 can see
            lim = cb.WGRAD_C * bound + 6e-8 * want.abs() + 1e-37
            assert bool((err > lim)[has_term].all()), "%s: losing h%sh%s stays inside 2e-5" % (case.id, drop[0], drop[1])
    nine = _emulate(case, nbr, kind, cb.KEPT + cb.DISCARDED)
    cb.within(nine, want, bound, c_piece, "%s %s, nine products" % (case.id, kind))
    lim = c_piece * bound + 6e-8 * want.abs() + 1e-37
    assert bool(((nine.double() - full.double()).abs() <= lim).all()), "%s: the discarded products move the result beyond the bound" % case.id


STEM_CASES = [c for c in cb.CASES if c.family == "stem_fp32"]


@pytest.mark.parametrize("case", STEM_CASES, ids=[c.id for c in STEM_CASES])
def test_stem_fp32_chain_against_the_abs_sum_bound(case):
    """The exact-fp32 chain in the kernel's order is the only arithmetic the small-map stem kernels may do: its own distance from
    float64 decides whether the project's constant can be asked of them (see the module docstring for the figures)."""
    case, nbr = cb.resolve(case)
    for kind in cb.KINDS:
        feats, w, gout = cb.operands(case, kind)
        want, bound = _want(case, kind)
        got = cb.fmaf_chain_wgrad(feats, gout, nbr) if case.op == "wgrad" else cb.fmaf_chain_fwd(feats, w, nbr)
        ratio, _ = cb.worst_ratio(got, want, bound, _c_of(case))
        print("fmaf chain %s %s: worst ratio %.3f" % (case.id, kind, ratio))
        c = STEM_FP32_BOUNDS.get((case.id, kind), _c_of(case))
        assert (ratio > 1.0) == ((case.id, kind) in STEM_FP32_BOUNDS), "%s %s: chain ratio %.2f, table out of date" % (case.id, kind, ratio)
        cb.within(got, want, bound, c, "%s %s, fp32 chain" % (case.id, kind))


def test_piece_aligned_pieces_are_what_the_name_says():
    g = torch.Generator().manual_seed(0)
    x = cb.adversarial("piece_aligned", 64, 8, g)
    h1, h2, h3 = cb.split3(x)
    assert torch.equal(h1 + h2 + h3, x) and bool((x > 0).all())
    assert torch.equal(h2, h1 * 2.0 ** -8) and torch.equal(h3, -h1 * 2.0 ** -17)
    w = cb.adversarial_weight("piece_aligned", 3, 8, 4, g, 1.0)
    p1, p2, p3 = cb.split3(w)
    assert torch.equal(p2, p1 * 2.0 ** -8) and torch.equal(p3, -p1 * 2.0 ** -17)


def test_the_split_and_the_six_products_are_stated_once():
    """csrc/split.h owns the arithmetic the bounds above describe: every split-bf16 convolution file takes its six products from
    split_products, nothing but split.h restates the scalar three-way split, and no per-site MFMA macro is left."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "openscene_amd", "csrc")
    texts = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    for f in ("spconv.hip", "spconv_tl.hip", "spconv_ws.hip", "spconv_rg.hip", "dense.hip", "wgrad_tl.hip", "stem.hip"):
        assert '#include "split.h"' in texts[f] and "split_products(" in texts[f], f
    assert [f for f, t in texts.items() if "- (float)h1" in t] == ["split.h"]
    for f, t in texts.items():
        assert not re.search(r"^\s*#\s*define\s+\w*MFMA\b", t, flags=re.M), f
