"""The reduced-precision modes of the four split-bf16 forward families on the device, through the ops.* wrappers (`pieces=`): the rg,
ws, tl and dense "fwd" cases of conv_bounds.CASES as they stand -- split and persistent tile-list launches, a one-row table, ragged
48-channel chunks, the out_rows permutation, swap and direct weight-stationary launches, 8 -> 20 and 768 -> 96 1x1 products, forward
and input-gradient weight images -- with the five operand kinds, NaN-padded inputs, for two pieces ("bf16x3") and one ("bf16x1"):

  * within FWD_C = 2e-6 of the abs-sum of the mode's own target (conv_pieces.target: the float64 sum of the kept products of the
    exact pieces).  test_conv_pieces_cpu.py shows what lands outside: a lost product (117 x and more), the six-product result
    (1.4 x and more on "wide_elements" at two pieces, 25 x and more on every kind at one piece);
  * within C2 = 2^-15 + 2e-6 / C1 = 2^-7 + 2e-6 of the abs-sum of the exact value (conv_pieces.C_EXACT);
  * a second call gives the same bits; a row without neighbours is exactly zero;
  * the tile-list case with bn=1: its per-tile batch-norm sums are those of the kernel's own output;
  * pieces = 3 through the `_pieces` entry gives the bits of the entry it sits beside.

Worst err / lim per family and mode over the family's cases and the five kinds, measured on an MI355X (own target | exact value):
    family   two pieces        one piece
    rg       0.35 | 0.47       0.19 | 0.99
    ws       0.38 | 0.52       0.19 | 0.99
    tl       0.54 | 0.47       0.28 | 0.99
    dense    0.66 | 0.61       0.34 | 0.99
(with the per-instance cases of conv_bounds.CASES: 96 -> 96 up to 384 -> 256 and the ragged 416 -> 128 on the tile-list kernel, 32 -> 32
up to 256 -> 256 on the weight-stationary one, 32 -> 32 register-gather, 64 -> 128 / 192 -> 128 / 384 -> 256 dense.)
(0.99 is "piece_aligned" at one piece: 0.992 of C1 by construction, as in the CPU emulation.)
"""
import pytest
import torch

import conv_bounds as cb
import conv_pieces as cp
from test_gpu_conv_bounds import dev, padded

pytestmark = pytest.mark.gpu

_LAUNCHES = {}


def launch_of(case):
    if case.id not in _LAUNCHES:
        rc, nbr = cb.resolve(case)
        _LAUNCHES[case.id] = (rc, nbr, cp.PiecesLaunch(rc, nbr, dev()))
    return _LAUNCHES[case.id]


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("pieces", [2, 1], ids=["bf16x3", "bf16x1"])
@pytest.mark.parametrize("case", cp.FWD_CASES, ids=cp.FWD_IDS)
def test_reduced_modes_meet_their_target_and_the_exact_bound(case, pieces):
    case, nbr, run = launch_of(case)
    d = dev()
    for kind in cb.KINDS:
        feats, w, _ = cb.operands(case, kind)
        ref = cb.reference(case, kind)
        want = cp.target(case, kind, pieces)
        label = "%s %s %s" % (case.id, kind, cp.MODES[pieces])
        fd, wd = padded(feats, d), w.to(d)
        part = None
        if case.opt.get("bn"):
            part = torch.zeros(run.tl.n_tiles, 2, case.cout, dtype=torch.float64, device=d)
        got = run.fwd(fd, wd, pieces, bn_partial=part)
        assert got.shape == ref.out.shape
        print("RATIO %s %s %s pieces=%d own %.3f exact %.3f" % (case.family, case.id, kind, pieces,
                                                                 cb.worst_ratio(got, want, ref.b_out, cb.FWD_C)[0],
                                                                 cb.worst_ratio(got, ref.out, ref.b_out, cp.C_EXACT[pieces])[0]))
        cb.within(got, want, ref.b_out, cb.FWD_C, label + " against its own target")
        cb.within(got, ref.out, ref.b_out, cp.C_EXACT[pieces], label + " against the exact value")
        assert _same_bits(got, run.fwd(fd, wd, pieces)), label + ": not bitwise reproducible"
        if nbr is not None and case.n_out > 3 and not case.opt.get("s2"):
            assert float(got[2].abs().max()) == 0.0, label + ": a row without neighbours is not exactly zero"
        if part is not None:                    # per-tile batch-norm sums against float64 column sums of the kernel's own output
            a = got.double()
            s1, s2 = part[:, 0].sum(0), part[:, 1].sum(0)
            assert (s1 - a.sum(0)).abs().max().item() <= 1e-9 * a.abs().sum(0).max().item(), label + ": bn_partial sums"
            assert (s2 - (a ** 2).sum(0)).abs().max().item() <= 1e-9 * (a ** 2).sum(0).max().item(), label + ": bn_partial squares"


@pytest.mark.parametrize("case", cp.FWD_CASES, ids=cp.FWD_IDS)
def test_three_pieces_through_the_new_entry_are_the_bits_of_the_old(case, monkeypatch):
    """ops.* sends pieces = 3 to the entry it always called; here the `_pieces` sibling is called with 3 instead."""
    from openscene_amd import ops
    case, nbr, run = launch_of(case)
    d = dev()
    feats, w, _ = cb.operands(case, "wide_elements")
    fd, wd = padded(feats, d), w.to(d)
    old = run.fwd(fd, wd, 3)
    lib = ops._prep(d)
    names = {"rg": "osn_spconv_fwd_rg", "ws": "osn_spconv_fwd_ws", "tl": "osn_spconv_fwd_tl", "dense": "osn_dense_fwd"}
    base = names[case.family]
    sibling = getattr(lib, base + "_pieces")
    called = []

    class Rerouted:
        def __getattr__(self, name):
            if name == base:
                return lambda *a: (called.append(name), sibling(*a, 3))[1]
            return getattr(lib, name)
    monkeypatch.setattr(ops, "_prep", lambda dev_: Rerouted())
    new = run.fwd(fd, wd, 3)
    assert called == [base]
    assert _same_bits(old, new), "%s: pieces = 3 through %s_pieces differs from %s" % (case.id, base, base)
    # ... and a reduced result differs from it (the argument reaches the kernel)
    monkeypatch.setattr(ops, "_prep", lambda dev_: lib)
    assert not _same_bits(old, run.fwd(fd, wd, 2)) and not _same_bits(old, run.fwd(fd, wd, 1))
