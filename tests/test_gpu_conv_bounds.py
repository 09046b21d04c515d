"""Every convolution kernel family against the per-element abs-sum bound of tests/conv_bounds.py, and isolated from the rows its
table does not name.  Each case calls the ops.* wrapper of the kernel its name says, on hand-made tables (about 30 % occupancy, 12 %
for the 125-offset stem, one output row without any neighbour, a tenth of the input rows referenced by nothing) or on the oracle's
2^3 stride-2 map, with the five operand kinds; a second call must be bitwise equal to the first.  test_conv_bounds_cpu.py shows
that these shapes and operands tell a kernel that loses one of its six cross products from one that keeps them.

Bounds: 2e-6 of the abs-sum for a forward / input-gradient launch, 2e-5 for a weight gradient, and 2e-6 for a weight gradient on
"piece_aligned" (conv_bounds.PIECE_WGRAD_C: at 2e-5 a lost h2h2 / h1h3 / h3h1 product cannot show).  The stem's exact-fp32 kernels
take no bound from the CPU chain: the chain meets the project's constants on every kind (figures: test_conv_bounds_cpu.py).

The cases are conv_bounds.CASES: per family the edge shapes, and per kernel INSTANCE a shipped network can launch the smallest shape
that reaches it (tile-list <NW, KS, ragged, OCC>, weight-stationary <NW, KS>, pair-array weight gradient <MB, NB>, the four
register-gather and dense instances, the first-generation forward and weight-gradient instances, the three stem forward kernels);
test_conv_census_cpu.py lists both sets without a GPU and fails when a network's instance has no case.

Worst err / lim per family and kind, measured on an MI355X (the assertion message prints the same figure):
(worst over the family's cases; forward rows against 2e-6, weight-gradient rows against 2e-5, last column against 2e-6)
    family          row_scales     cancellation   gradient_sized wide_elements  piece_aligned  piece@2e-6
    rg fwd          0.14           0.01           0.06           0.19           0.46           -
    stem_fp32 fwd   0.23           0.08           0.12           0.27           0.26           -
    stem_fp32 wgrad 0.02           0.01           0.01           0.02           0.02           0.17
    stem_mfma fwd   0.18           0.09           0.10           0.20           0.28           -
    stem_mfma wgrad 0.01           0.00           0.00           0.01           0.01           0.13
    ws fwd          0.10           0.01           0.12           0.29           0.58           -
    tl fwd          0.24           0.01           0.14           0.42           0.72           -
    wgrad_tl wgrad  0.04           0.04           0.01           0.04           0.05           0.51
    wgrad1 wgrad    0.04           0.04           0.01           0.05           0.08           0.74
    dense fwd       0.12           0.02           0.12           0.32           0.93           -
    x6 fwd          0.14           0.01           0.13           0.30           0.65           -
Where each family's worst sits: rg 64 -> 64 at K = 125; ws 256 -> 128 on the stride-2 map (swap); tl the persistent 32 -> 512 launch
(the widest shapes: 384 -> 256 0.35, 416 -> 128 0.37); wgrad_tl 64 -> 20; wgrad1 the 64 -> 768 head; dense 768 -> 96 (384 -> 256:
0.65); x6 128 -> 64 at 32 800 rows.
"""
import hashlib

import numpy as np
import pytest
import torch

import conv_bounds as cb

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


_LAUNCHES = {}


def launch_of(case):
    if case.id not in _LAUNCHES:
        rc, nbr = cb.resolve(case)
        _LAUNCHES[case.id] = (rc, nbr, cb.Launch(rc, nbr, dev()))
    return _LAUNCHES[case.id]


def padded(x, d):
    """x as the leading rows of a larger NaN-filled allocation on the device: a read past the last row does not stay unseen."""
    big = torch.full((x.shape[0] + 64, x.shape[1]), float("nan"), dtype=torch.float32, device=d)
    big[:x.shape[0]] = x.to(d)
    return big[:x.shape[0]]


def _sha(t):
    """sha256 of a tensor's bytes: the BITS lines are what two builds of the library are compared by."""
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("case", cb.CASES, ids=cb.CASE_IDS)
def test_per_element_abs_sum_bound(case):
    case, nbr, run = launch_of(case)
    d = dev()
    for kind in cb.KINDS:
        feats, w, gout = cb.operands(case, kind)
        ref = cb.reference(case, kind)
        label = "%s %s" % (case.id, kind)
        fd = padded(feats, d)
        if case.op == "wgrad":
            gd = padded(gout, d)
            got = run.wgrad(fd, gd)
            assert got.shape == ref.gw.shape
            print("BITS %s %s %s" % (case.id, kind, _sha(got)))
            ratio, n_bad = cb.worst_ratio(got, ref.gw, ref.b_gw, cb.WGRAD_C)
            print("RATIO %s %s %s %.3f" % (case.family, case.id, kind, ratio))
            if kind == "piece_aligned":
                print("RATIO %s %s %s@2e-6 %.3f" % (case.family, case.id, kind, cb.worst_ratio(got, ref.gw, ref.b_gw, cb.PIECE_WGRAD_C)[0]))
            cb.within(got, ref.gw, ref.b_gw, cb.WGRAD_C, label + " weight gradient")
            if kind == "piece_aligned":
                cb.within(got, ref.gw, ref.b_gw, cb.PIECE_WGRAD_C, label + " weight gradient at the piece bound")
            assert torch.equal(got, run.wgrad(fd, gd)), label + ": not bitwise reproducible"
            continue
        wd = w.to(d)
        part = None
        if case.opt.get("bn"):
            part = torch.zeros(run.tl.n_tiles, 2, case.cout, dtype=torch.float64, device=d)
        got = run.fwd(fd, wd, bn_partial=part) if part is not None else run.fwd(fd, wd)
        assert got.shape == ref.out.shape
        print("BITS %s %s %s" % (case.id, kind, _sha(got)))
        print("RATIO %s %s %s %.3f" % (case.family, case.id, kind, cb.worst_ratio(got, ref.out, ref.b_out, cb.FWD_C)[0]))
        cb.within(got, ref.out, ref.b_out, cb.FWD_C, label + " forward")
        assert torch.equal(got, run.fwd(fd, wd)), label + ": not bitwise reproducible"
        if nbr is not None and case.n_out > 3 and not case.opt.get("s2"):
            assert float(got[2].abs().max()) == 0.0, label + ": a row without neighbours is not exactly zero"
        if part is not None:                    # per-tile batch-norm sums against float64 column sums of the kernel's own output
            a = got.double()
            s1, s2 = part[:, 0].sum(0), part[:, 1].sum(0)
            assert (s1 - a.sum(0)).abs().max().item() <= 1e-9 * a.abs().sum(0).max().item(), label + ": bn_partial sums"
            assert (s2 - (a ** 2).sum(0)).abs().max().item() <= 1e-9 * (a ** 2).sum(0).max().item(), label + ": bn_partial squares"


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("case", cb.CASES, ids=cb.CASE_IDS)
def test_rows_the_table_does_not_name_stay_out(case):
    """inf / NaN in input rows that no table entry references (and, for a weight gradient, in the gradient rows of output rows without
    a pair) change no bit of the result; inf / NaN in ONE referenced input row reach exactly the output rows (weight gradient: the
    offsets) that reference it, and every other element keeps its bits.  All indices stay inside their allocations."""
    case, nbr, run = launch_of(case)
    d = dev()
    feats, w, gout = cb.operands(case, "row_scales")
    table = nbr if nbr is not None else np.arange(case.n_in, dtype=np.int32)[None]
    used = np.zeros(case.n_in, dtype=bool)
    used[table[table >= 0]] = True
    unref = np.nonzero(~used)[0]
    if nbr is not None:
        assert unref.shape[0] >= 0.05 * case.n_in, "%s: only %d of %d input rows are unreferenced" % (case.id, unref.shape[0], case.n_in)
    no_pair = np.nonzero((table < 0).all(0))[0]
    wd = w.to(d)

    def result(f, g_):
        fd = padded(f, d)
        return run.wgrad(fd, padded(g_, d)) if case.op == "wgrad" else run.fwd(fd, wd)

    clean = result(feats, gout)
    assert bool(torch.isfinite(clean).all())
    poison = torch.tensor([float("inf"), float("nan"), float("-inf")])
    f2, g2 = feats.clone(), gout.clone()
    if unref.shape[0]:
        f2[torch.from_numpy(unref)] = poison[torch.arange(unref.shape[0] * case.cin) % 3].reshape(unref.shape[0], case.cin)
    if case.op == "wgrad" and no_pair.shape[0]:
        g2[torch.from_numpy(no_pair)] = poison[torch.arange(no_pair.shape[0] * case.cout) % 3].reshape(no_pair.shape[0], case.cout)
    assert _same_bits(clean, result(f2, g2)), "%s: a row that no table entry names reached the result" % case.id

    r = int(np.nonzero(used)[0][len(np.nonzero(used)[0]) // 2])            # one referenced row
    f3 = feats.clone()
    f3[r] = float("inf")
    got = result(f3, gout).cpu()
    if case.op == "wgrad":
        hit = torch.from_numpy((table == r).any(1))                       # offsets under which row r appears
        assert hit.shape[0] == got.shape[0]
    else:
        hit = torch.from_numpy((table == r).any(0))                       # output rows that reference row r
    flat = got.reshape(got.shape[0], -1)
    assert bool(hit.any())
    assert torch.equal(~torch.isfinite(flat).all(1), hit), "%s: the non-finite %s are not those that reference the poisoned row" % (
        case.id, "offsets" if case.op == "wgrad" else "rows")
    assert not bool(torch.isfinite(flat[hit]).any()), "%s: finite elements where the poisoned row contributes" % case.id
    assert _same_bits(flat[~hit], clean.cpu().reshape(got.shape[0], -1)[~hit]), "%s: elements away from the poisoned row changed" % case.id
