"""The reduced-precision pair-array weight gradient on the device, through ops.spconv_wgrad_tl(pieces=) and the C entries: every case
of train_pieces.WGRAD_CASES -- all nine <MB, NB> blockings, widths past one workgroup tile, the K = 8 swap launches on the stride-2
maps, identity maps, one output row (every step padded, empty offsets) -- with the five operand kinds, NaN-padded operands, for two
pieces ("bf16x3") and one ("bf16x1"):

  * within WGRAD_C (PIECE_WGRAD_C on "piece_aligned") of the abs-sum of the mode's own target (train_pieces.target: the float64 sum
    of the kept products of the exact pieces); test_train_pieces_cpu.py shows what lands outside;
  * within 2^-15 / 2^-7 + WGRAD_C of the abs-sum of the exact value (train_pieces.C_EXACT);
  * different bits from the three-piece result (the argument reached the kernel; "piece_aligned" at two pieces excepted, see the
    test), the same bits from a second call;
  * pieces = 3 through the `_pieces` entry gives the bits of the entry it sits beside;
  * partial launches + the batched reduction give the bits of the one-call entry, in every mode.

(The tile-list forward case with batch-norm partial sums, conv_pieces.FWD_CASES' bn=1 case, runs reduced in test_gpu_conv_pieces.py.)

Worst err / lim over the 21 cases and the five kinds, measured on an MI355X (own target | exact value):
    two pieces   0.39 | 0.54        one piece   0.23 | 0.99
(0.99 is "piece_aligned" at one piece: tight by construction, as in the forward families.)
"""
import pytest
import torch

import conv_bounds as cb
import conv_pieces as cp
import train_pieces as tp
from test_gpu_conv_bounds import dev, padded

pytestmark = pytest.mark.gpu

_LAUNCHES = {}


def launch_of(case):
    if case.id not in _LAUNCHES:
        rc, nbr = cb.resolve(case)
        _LAUNCHES[case.id] = (rc, nbr, tp.WgradLaunch(rc, nbr, dev()))
    return _LAUNCHES[case.id]


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("pieces", [2, 1], ids=["bf16x3", "bf16x1"])
@pytest.mark.parametrize("case", tp.WGRAD_CASES, ids=tp.WGRAD_IDS)
def test_reduced_weight_gradient_meets_its_target_and_the_exact_bound(case, pieces):
    case, nbr, run = launch_of(case)
    d = dev()
    for kind in cb.KINDS:
        feats, _, gout = cb.operands(case, kind)
        ref = cb.reference(case, kind)
        want = tp.target(case, kind, pieces)
        label = "%s %s %s" % (case.id, kind, cp.MODES[pieces])
        fd, gd = padded(feats, d), padded(gout, d)
        got = run.wgrad(fd, gd, pieces)
        assert got.shape == ref.gw.shape
        print("RATIO wgrad_tl %s %s pieces=%d own %.3f exact %.3f" % (case.id, kind, pieces,
                                                                      cb.worst_ratio(got, want, ref.b_gw, tp.c_own(kind))[0],
                                                                      cb.worst_ratio(got, ref.gw, ref.b_gw, tp.C_EXACT[pieces])[0]))
        cb.within(got, want, ref.b_gw, tp.c_own(kind), label + " against its own target")
        cb.within(got, ref.gw, ref.b_gw, tp.C_EXACT[pieces], label + " against the exact value")
        assert _same_bits(got, run.wgrad(fd, gd, pieces)), label + ": not bitwise reproducible"
        # ("piece_aligned" at two pieces may legitimately give the three-piece bits: every element has the mantissa
        #  1 + 2^-8 - 2^-17 times a power of two, so per pair the dropped products are 2^-16 - 2^-17 - 2^-17 = 0 exactly --
        #  with one pair per offset, the one-row case, they are added as an exact zero.  The other four kinds decide at two pieces.)
        if not (kind == "piece_aligned" and pieces == 2):
            assert not _same_bits(got, run.wgrad(fd, gd, 3)), label + ": the bits of the three-piece result (the mode reached no kernel)"


@pytest.mark.parametrize("case", tp.WGRAD_CASES, ids=tp.WGRAD_IDS)
def test_three_pieces_through_the_new_entry_are_the_bits_of_the_old(case, monkeypatch):
    """ops.spconv_wgrad_tl sends pieces = 3 to the entry it always called; here the `_pieces` sibling is called with 3 instead."""
    from openscene_amd import ops
    case, nbr, run = launch_of(case)
    d = dev()
    feats, _, gout = cb.operands(case, "wide_elements")
    fd, gd = padded(feats, d), padded(gout, d)
    old = run.wgrad(fd, gd, 3)
    lib = ops._prep(d)
    called = []

    class Rerouted:
        def __getattr__(self, name):
            if name == "osn_spconv_wgrad_tl":
                return lambda *a: (called.append(name), lib.osn_spconv_wgrad_tl_pieces(*a, 3))[1]
            return getattr(lib, name)
    monkeypatch.setattr(ops, "_prep", lambda dev_: Rerouted())
    new = run.wgrad(fd, gd, 3)
    assert called == ["osn_spconv_wgrad_tl"]
    assert _same_bits(old, new), "%s: pieces = 3 through osn_spconv_wgrad_tl_pieces differs from osn_spconv_wgrad_tl" % case.id


@pytest.mark.parametrize("pieces", [3, 2, 1], ids=["bf16x6", "bf16x3", "bf16x1"])
def test_partial_launches_and_the_batched_reduction_are_the_bits_of_the_one_call_entry(pieces):
    d = dev()
    entries, single = [], []
    for i, case in enumerate(tp.WGRAD_CASES):
        rc, _nbr, run = launch_of(case)
        feats, _, gout = cb.operands(rc, cb.KINDS[i % len(cb.KINDS)])
        fd, gd = padded(feats, d), padded(gout, d)
        entries.append((run, fd, gd))
        single.append(run.wgrad(fd, gd, pieces))
    got = tp.batched_wgrad(entries, d, pieces)
    for (run, _f, _g), a, b in zip(entries, single, got):
        assert _same_bits(a, b), "%s, %d pieces: partial + batched reduction differs from the one-call entry" % (run.case.id, pieces)
    if pieces == 3:             # ... and the old partial entry gives the same jobs' results
        old, _jobs = cb.batched_wgrad(entries, d)
        for (run, _f, _g), a, b in zip(entries, old, got):
            assert _same_bits(a, b), "%s: osn_spconv_wgrad_tl_partial_pieces(3) differs from osn_spconv_wgrad_tl_partial" % run.case.id
