"""Reduced-precision TRAINING ("bf16x3" / "bf16x1" through the backward pass) without a GPU.

The pair-array weight gradient, with conv_bounds.split_emulation(..., wgrad=True) standing in for the kernel, on every case of
train_pieces.WGRAD_CASES and the five operand kinds:

  * the emulation meets both bounds of its mode (train_pieces: own target within WGRAD_C, within PIECE_WGRAD_C on "piece_aligned";
    exact value within 2^-15 / 2^-7 + WGRAD_C);
  * on "piece_aligned" a two-piece sum that loses "21" or "12", a one-piece sum that loses its only product, and the six-product
    result taken for a ONE-piece one fall outside the own-target bound.  The six-product result taken for a TWO-piece one does not,
    on this kind: with both operands at the mantissa 1 + 2^-8 - 2^-17 the dropped products cancel (22 = 2^-16, 13 + 31 = -2^-16), as
    test_conv_pieces_cpu.py found for the forward -- asserted as such, so the statement stays honest; the GPU test asks for a bitwise
    difference from the three-piece result instead.

Then the host side: header, ctypes table and exports of the two new entries and the two new osn_net_run flag bits, bad `pieces`, the flag
table of osn_net_forward / osn_net_backward (checked before any launch: the all-zero descriptor is what fails next), the launches of a
reduced training step on both host paths under the null HIP runtime of tools/dryrun, and the `train_precision` knob of
openscene_amd.precision.
"""
import ctypes
import os
import re
import threading

import pytest
import torch

import conv_bounds as cb
import conv_pieces as cp
import train_pieces as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True, scope="module")
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 8))
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("case", tp.WGRAD_CASES, ids=tp.WGRAD_IDS)
def test_emulated_weight_gradient_meets_both_bounds_and_mistakes_do_not(case):
    case, nbr = cb.resolve(case)
    for kind in cb.KINDS:
        ref = cb.reference(case, kind)
        six = tp.emulate(case, nbr, kind, cp.KEEP[3]) if kind == "piece_aligned" else None
        for pieces in (2, 1):
            want = tp.target(case, kind, pieces)
            got = tp.emulate(case, nbr, kind, cp.KEEP[pieces])
            label = "%s %s, %d pieces" % (case.id, kind, pieces)
            r_own = cb.within(got, want, ref.b_gw, tp.c_own(kind), label + " against its target")
            r_exact = cb.within(got, ref.gw, ref.b_gw, tp.C_EXACT[pieces], label + " against the exact value")
            print("EMU %s %s pieces=%d own %.3f exact %.3f" % (case.id, kind, pieces, r_own, r_exact))
            if kind != "piece_aligned":
                continue
            # one kept product removed
            for drop in cp.KEEP[pieces]:
                if drop == "11" and pieces == 2:
                    continue                                   # (losing the leading product is not a subtle mistake)
                lost = tp.emulate(case, nbr, kind, [ij for ij in cp.KEEP[pieces] if ij != drop])
                d = tp.distance(lost, want, ref.b_gw, kind)
                print("LOST %s pieces=%d h%sh%s distance %.1f" % (case.id, pieces, drop[0], drop[1], d))
                assert d > 1.0, "%s: a lost h%sh%s sits only %.2f x the bound from the target" % (label, drop[0], drop[1], d)
            # `pieces` ignored: the six-product result
            d_six = tp.distance(six, want, ref.b_gw, kind)
            print("SIX %s pieces=%d distance %.2f" % (case.id, pieces, d_six))
            if pieces == 1:
                assert d_six > 1.0, "%s: six products only %.2f x the bound from the one-piece target" % (label, d_six)
            else:
                assert d_six < 1.0, "%s: piece_aligned was not expected to tell six products from three (%.2f)" % (label, d_six)


def test_bounds_follow_their_derivation():
    assert tp.C_EXACT == {3: cb.WGRAD_C, 2: 2.0 ** -16 + 2 * 2.0 ** -17 + cb.WGRAD_C, 1: 2 * 2.0 ** -8 + cb.WGRAD_C}
    assert tp.c_own("piece_aligned") == cb.PIECE_WGRAD_C and all(tp.c_own(k) == cb.WGRAD_C for k in cb.KINDS if k != "piece_aligned")
    assert set(tp.WGRAD_IDS) == {c.id for c in cb.CASES if c.family == "wgrad_tl"} | {tp.ONE_ROW.id}
    one, nbr = cb.resolve(tp.ONE_ROW)
    counts = (nbr >= 0).sum(1)
    assert one.n_out == 1 and counts.max() <= 1 and (counts == 0).any() and (counts == 1).any()      # padded steps, empty offsets


# ------------------------------------------------------------------------------------------------------------ the C ABI
NEW_ENTRIES = {"osn_spconv_wgrad_tl_pieces": "osn_spconv_wgrad_tl", "osn_spconv_wgrad_tl_partial_pieces": "osn_spconv_wgrad_tl_partial"}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from openscene_amd import _lib
    return _lib.load()


def test_header_ctypes_and_exports_agree_on_the_new_names(lib):
    from openscene_amd import _lib
    src = open(os.path.join(ROOT, "include", "openscene_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, base in NEW_ENTRIES.items():
        assert hasattr(lib, name), name                                         # exported by the built library
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code, flags=re.S).group(1)
        base_decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % base, code, flags=re.S).group(1)
        norm = lambda t: [re.sub(r"\s+", " ", a).strip() for a in t.split(",")]
        assert norm(decl) == norm(base_decl) + ["int pieces"], name
        assert _lib.PROTOTYPES[name] == (_lib.PROTOTYPES[base][0], _lib.PROTOTYPES[base][1] + [ctypes.c_int]), name
    assert re.search(r"#define\s+OSN_NET_RUN_TRAIN_PIECES_2\s+16\b", src) and re.search(r"#define\s+OSN_NET_RUN_TRAIN_PIECES_1\s+32\b", src)
    assert re.search(r"#define\s+OSN_NET_RUN_PIECES_2\s+4\b", src) and re.search(r"#define\s+OSN_NET_RUN_PIECES_1\s+8\b", src)      # untouched
    assert lib.osn_version() == 3                                               # additive: nothing bumped


def test_pieces_out_of_range_is_refused_before_anything_else(lib):
    from openscene_amd import _lib
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 15) & ~15
    job = (ctypes.c_char * 40)()
    for bad in (0, 4, -1):
        # (every other argument is one the base entry would refuse as well: null job, cin = 3)
        assert lib.osn_spconv_wgrad_tl_pieces(None, None, None, 0, None, 8, 8, 27, 3, 3, None, 0, None, bad) == -1
        assert _lib.last_error().startswith("osn_spconv_wgrad_tl_pieces: pieces=%d" % bad), _lib.last_error()
        assert lib.osn_spconv_wgrad_tl_partial_pieces(None, None, None, 0, None, 8, 8, 27, 3, 3, None, 0, None, None, bad) == -1
        assert _lib.last_error().startswith("osn_spconv_wgrad_tl_partial_pieces: pieces=%d" % bad), _lib.last_error()
    for ok in (1, 2, 3):
        # a valid piece count goes on to the entry's own checks
        assert lib.osn_spconv_wgrad_tl_pieces(p, p, None, 0, p, 8, 8, 27, 3, 32, p, 4096, None, ok) == -1
        assert "pieces" not in _lib.last_error() and _lib.last_error().startswith("osn_spconv_wgrad_tl: needs cin"), _lib.last_error()
        assert lib.osn_spconv_wgrad_tl_partial_pieces(p, p, None, 0, p, 8, 8, 27, 32, 32, p, 4096, None, None, ok) == -1
        assert _lib.last_error().startswith("osn_spconv_wgrad_tl_partial: null job"), _lib.last_error()
        assert lib.osn_spconv_wgrad_tl_partial_pieces(p, p, None, 0, p, 8, 8, 27, 3, 32, p, 4096, ctypes.addressof(job), None, ok) == -1
        assert _lib.last_error().startswith("osn_spconv_wgrad_tl: needs cin"), _lib.last_error()


def test_net_run_training_flags_are_checked_before_the_first_launch(lib):
    from openscene_amd import _lib, executor as E
    assert E.RUN_TRAIN_PIECES == {3: 0, 2: 16, 1: 32} and E.RUN_PIECES == {3: 0, 2: 4, 1: 8}
    desc = E._Desc()                                   # all zero: any call that gets past the flag check fails on the descriptor

    def call(fn, flags, training):
        run = E._Run()
        run.flags, run.training = flags, training
        rc = fn(ctypes.addressof(desc), ctypes.addressof(run), None)
        return rc, _lib.last_error()

    for flags in (16 | 32, 4 | 16, 8 | 32, 4 | 32, 8 | 16):
        for training in (0, 1):
            rc, msg = call(lib.osn_net_forward, flags, training)
            assert rc == -1 and msg.startswith("osn_net_forward: flags %d" % flags), (flags, training, msg)
        rc, msg = call(lib.osn_net_backward, flags, 1)
        assert rc == -1 and msg.startswith("osn_net_backward: flags %d" % flags), (flags, msg)
    for flags in (16, 32, 16 | 1, 32 | 2):
        for fn, training in ((lib.osn_net_forward, 0), (lib.osn_net_forward, 1), (lib.osn_net_backward, 1)):
            rc, msg = call(fn, flags, training)
            assert rc == -1 and "flags" not in msg, (flags, training, msg)       # past the flag check: the zero descriptor is what fails


def test_kernel_text_takes_its_plane_count_from_the_piece_count():
    csrc = os.path.join(ROOT, "openscene_amd", "csrc")
    code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "wgrad_tl_kernel.h")).read())
    assert "split_products<NP>(" in code and "split_products(" not in code and "tl_split4<NP>(" in code
    assert re.search(r"Ap\[NP\]\[32\]", code) and re.search(r"Gp\[NP\]\[32\]", code) and re.search(r"fa\[MB\]\[NP\]", code)
    assert not re.search(r"\]\[3\];|pl < 3\b", code)
    hip = open(os.path.join(csrc, "wgrad_tl.hip")).read()
    assert hip.count('#include "wgrad_tl_kernel.h"') == 2                      # the three-piece kernel and the reduced template
    assert "#define OSN_WG_NAME wgrad_tl_kernel\n" in hip and "#define OSN_WG_NAME wgrad_tl_pieces_kernel\n" in hip


# ------------------------------------------------------------------------------------------------------------ the launches of a step
@pytest.mark.parametrize("mode,np_", [("bf16x3", 2), ("bf16x1", 1)])
def test_dry_run_training_step_launches_reduced_instances_on_both_host_paths(mode, np_, monkeypatch):
    """One training step of MinkUNet18A with the null HIP runtime of tools/dryrun (every launch becomes a log line): in a reduced mode
    the executor and the module path issue the same convolution launches, every launch of the four forward families (forward and
    input gradient) and every pair-array weight gradient is the instance with the mode's piece count, and the stem's
    forward and weight gradient are the kernels they always were."""
    import collections
    import sys
    import openscene_amd as osn
    sys.path.insert(0, os.path.join(ROOT, "tools", "dryrun"))
    import dry_step
    lib = dry_step.install(dry_step.build_dry_lib(), monkeypatch.setattr)
    base = osn.set_train_precision(mode)
    try:
        logs, _step, sizes = dry_step.step_logs(lib, "MinkUNet18A", points=12000, setattr_=monkeypatch.setattr)
    finally:
        osn.set_train_precision(base)
    a, b = dry_step.conv_launches(logs["modules"]), dry_step.conv_launches(logs["executor"])
    assert len(a) > 100 and collections.Counter(a) == collections.Counter(b)
    for text in (logs["modules"], logs["executor"]):           # (every launch: the 1x1 kernel is not among conv_launches)
        for fam in ("spconv_tl", "spconv_ws", "spconv_rg", "dense", "wgrad_tl"):
            # (a name is demangled "fam_kernel<2, ..." or, where c++filt does not know a bf16 argument type, left "fam_kernelILi2E...")
            assert not re.search(r"%s_kernel(<|I)" % fam, text), "%s: a three-piece %s launch in a %s step" % (mode, fam, mode)
            other = [m for m in re.findall(r"%s_pieces_kernel(?:<|ILi)(\d)" % fam, text) if int(m) != np_]
            assert not other, (fam, other)
        count = lambda fam: len(re.findall(r"%s_pieces_kernel(?:<|ILi)%d" % (fam, np_), text))
        assert count("wgrad_tl") >= 20 and count("spconv_tl") >= 4 and count("dense") >= 2
        assert "stem_fwd" in text and "stem_wgrad_kernel" in text            # exact in every mode: the stem, forward and weight gradient


# ------------------------------------------------------------------------------------------------------------ the mode selector
def test_train_precision_semantics():
    import openscene_amd as osn
    from openscene_amd import precision
    assert osn.train_precision is precision.train_precision and osn.set_train_precision is precision.set_train_precision
    assert osn.get_train_precision is precision.get_train_precision
    base = osn.get_train_precision()
    try:
        assert osn.set_train_precision("bf16x6") == base
        assert osn.get_train_precision() == "bf16x6" and precision.pass_pieces(True, True) == 3
        with osn.train_precision("bf16x3"):
            assert osn.get_train_precision() == "bf16x3"
            with osn.train_precision("bf16x1"):
                assert osn.get_train_precision() == "bf16x1"
                with osn.train_precision("bf16x6"):
                    assert precision.pass_pieces(True, False) == 3
                assert osn.get_train_precision() == "bf16x1"
            assert osn.get_train_precision() == "bf16x3"
        assert osn.get_train_precision() == "bf16x6"
        with pytest.raises(RuntimeError):
            with osn.train_precision("bf16x1"):
                raise RuntimeError("body")
        assert osn.get_train_precision() == "bf16x6"                             # restored on an exception
        for bad in ("bf16x2", "fp16", "", None, 3):
            with pytest.raises(ValueError):
                osn.train_precision(bad)
            with pytest.raises(ValueError):
                osn.set_train_precision(bad)
        assert osn.get_train_precision() == "bf16x6"
        # the process default, and a context over it; another thread sees the default, not this thread's context
        assert osn.set_train_precision("bf16x1") == "bf16x6" and precision.pass_pieces(True, True) == 1
        with osn.train_precision("bf16x3"):
            seen = []
            t = threading.Thread(target=lambda: seen.append(osn.get_train_precision()))
            t.start()
            t.join()
            assert seen == ["bf16x1"] and osn.get_train_precision() == "bf16x3"
        assert osn.get_train_precision() == "bf16x1"
    finally:
        osn.set_train_precision(base)
    # the initial default: OSN_TRAIN_PRECISION, read by Python; OSN_INFER_PRECISION is the other knob's
    assert precision._initial_train({}) == "bf16x6" and precision._initial_train({"OSN_TRAIN_PRECISION": ""}) == "bf16x6"
    assert precision._initial_train({"OSN_TRAIN_PRECISION": "bf16x3"}) == "bf16x3"
    assert precision._initial_train({"OSN_INFER_PRECISION": "bf16x1"}) == "bf16x6"
    assert precision._initial({"OSN_TRAIN_PRECISION": "bf16x1"}) == "bf16x6"
    with pytest.raises(ValueError):
        precision._initial_train({"OSN_TRAIN_PRECISION": "fast"})


def test_pass_pieces_table_and_the_independence_of_the_two_knobs():
    import openscene_amd as osn
    from openscene_amd import precision
    pieces = {"bf16x6": 3, "bf16x3": 2, "bf16x1": 1}
    b_inf, b_tr = osn.set_conv_precision("bf16x6"), osn.set_train_precision("bf16x6")
    try:
        for inf in pieces:
            for tr in pieces:
                with osn.conv_precision(inf), osn.train_precision(tr):
                    assert osn.get_conv_precision() == inf and osn.get_train_precision() == tr
                    assert precision.pass_pieces(False, False) == pieces[inf]             # evaluation mode, no graph: the inference mode
                    for training, grad in ((True, False), (False, True), (True, True)):
                        assert precision.pass_pieces(training, grad) == pieces[tr]        # everything else: the training mode
                    # inference_pieces keeps its meaning: the inference mode or 3
                    assert precision.inference_pieces(False, False) == pieces[inf]
                    assert precision.inference_pieces(True, False) == precision.inference_pieces(False, True) == 3
                assert osn.get_conv_precision() == "bf16x6" and osn.get_train_precision() == "bf16x6"
        # the process defaults are independent too
        osn.set_train_precision("bf16x1")
        assert osn.get_conv_precision() == "bf16x6" and precision.pass_pieces(False, False) == 3 and precision.pass_pieces(True, True) == 1
        osn.set_train_precision("bf16x6")
        osn.set_conv_precision("bf16x1")
        assert osn.get_train_precision() == "bf16x6" and precision.pass_pieces(True, True) == 3 and precision.pass_pieces(False, False) == 1
    finally:
        osn.set_conv_precision(b_inf)
        osn.set_train_precision(b_tr)


def test_wrappers_take_pieces_and_the_default_mode_calls_the_old_entry():
    import inspect
    from openscene_amd import ops
    assert inspect.signature(ops.spconv_wgrad_tl).parameters["pieces"].default == 3
    for bad in (0, 4, None):
        with pytest.raises(ValueError):
            ops.spconv_wgrad_tl(torch.zeros(4, 8), torch.zeros(4, 8), None, 1, pieces=bad)
    src = inspect.getsource(ops.spconv_wgrad_tl)
    assert "if pieces == 3:\n            check(lib.osn_spconv_wgrad_tl(*args)" in src
