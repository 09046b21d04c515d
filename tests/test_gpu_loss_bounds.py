"""The distillation loss (csrc/loss.hip, through losses.distill_loss only) against the per-element and per-loss limits of
tests/loss_bounds.py, at the edges of the kernels' own loops -- the 256-column step of a wave from one lane (d = 4) to five steps, the
four rows per workgroup, the 1024 threads of the mean -- on Gaussian rows, rows ALIGNED with their target (the regime training moves
into: the two terms of the cosine gradient cancel), columns spread over six decades and rows on both sides of the eps = 1e-8 clamp,
always with an UNSORTED selection (one case sorted), at three upstream gradients.  test_loss_bounds_cpu.py shows that these limits
separate the kernels' arithmetic (ratio <= 0.5) from eight single defects, six of which the criteria of test_gpu_dense.py let pass.

Also: the L1 gradient bit by bit; bitwise repeatability of the loss and of the gradient; the compacted rows and the inverse table that
travel with the gradient to the network executor; the clamp rows; and the isolation of rows under non-finite values.  A small
pass-through autograd.Function in front of the loss captures the gradient tensor and its `_osn_rows` hint as the executor receives them.

Worst err / limit per kind and quantity, measured on an MI355X (the "RATIO" lines, all shapes and upstream gradients; the numpy
emulation of test_loss_bounds_cpu.py in brackets -- the device contracts a * b + c into an fma, the emulation rounds twice):
    cosine  gauss    gradient 0.175 (0.169)   loss 0.014 (0.014)
    cosine  aligned  gradient 0.146 (0.157)   loss 0.020 (0.020)
    cosine  decades  gradient 0.194 (0.194)   loss 0.018 (0.018)
    cosine  clamp    gradient 0.177 (0.177)   loss 0.014 (0.014)
    l1      gauss    gradient bit by bit      loss 0.073
    rows outside sel: +0 in every case

FOUND with the first run of test_cosine_a_non_finite_value_stays_in_its_row: the kernels clamped the norms with fmaxf, which returns
its OTHER operand for a NaN -- a NaN in a selected output row gave a NaN loss but kb = s / (eps nb), so the row's gradient was the
finite, 1e8-sized b / (eps nb) in every element but the NaN's own.  csrc/loss.hip now clamps with `r <= eps ? eps : r`, which keeps
the NaN (the same bits for every other r).
"""
import numpy as np
import pytest
import torch

import loss_bounds as lb

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.array(a)).to(dev())                # (a copy: the shared inputs are read-only)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class _Tap(torch.autograd.Function):
    """Identity in front of the loss: its backward sees the gradient tensor distill_loss returned, attributes included."""

    @staticmethod
    def forward(ctx, x, box):
        ctx.box = box
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        ctx.box["grad"] = g
        ctx.box["hint"] = getattr(g, "_osn_rows", None)
        return g, None


class Run:
    """One forward pass of distill_loss on device copies of (out, sel, target); backward(up) -> (gradient tensor, hint)."""

    def __init__(self, out, sel, target, loss_type):
        from openscene_amd.losses import distill_loss
        self.box = {}
        self.x = (out if torch.is_tensor(out) else _t(out)).clone().requires_grad_(True)
        self.sel = sel if torch.is_tensor(sel) else _t(sel)
        self.target = target if torch.is_tensor(target) else _t(target)
        self.loss = distill_loss(_Tap.apply(self.x, self.box), self.sel, self.target, loss_type)

    def backward(self, up=1.0):
        self.x.grad = None
        self.box.clear()
        (self.loss * up).backward(retain_graph=True)
        return self.box["grad"], self.box["hint"]


def _check(run, cs, label, worst):
    """Loss and gradient within the limits at every upstream gradient of lb.UPS; -> {up: gradient (numpy)}."""
    grads = {}
    for up in lb.UPS:
        r = lb.reference(cs.out, cs.sel, cs.target, cs.loss_type, up)
        g, hint = run.backward(up)
        assert (hint is None) == (cs.n_sel == cs.n), "%s: the row hint is attached exactly when n_sel < n" % label
        grads[up] = g.cpu().numpy()
        flat = lb.within({"loss": run.loss.item(), "grad": grads[up]}, r, lb.limits(r), "%s up %g" % (label, up), worst)
        print("RATIO %s up %g %s" % (label, up, "  ".join("%s %.3f" % kv for kv in sorted(flat.items()))))
    return grads


CASES = [(k, n, n_sel, d) for (n, n_sel, d) in lb.SHAPES for k in lb.KINDS]
IDS = ["%s-%dof%dx%d" % (k, n_sel, n, d) for (k, n, n_sel, d) in CASES]


@pytest.mark.parametrize("kind,n,n_sel,d", CASES, ids=IDS)
def test_cosine_loss_and_gradient_within_the_limits(kind, n, n_sel, d):
    cs = lb.case(kind, n, n_sel, d)
    worst = {}
    grads = _check(Run(cs.out, cs.sel, cs.target, "cosine"), cs, "cosine %s %d of %d x %d" % (kind, n_sel, n, d), worst)
    if kind == "clamp":                                      # finite on every degenerate row; a zero target row: a zero gradient
        assert np.isfinite(grads[1.0]).all()
        zero_b = ~cs.target.any(axis=1)
        assert (zero_b.any() or n_sel < 4) and not grads[1.0][cs.sel[zero_b]].any()
    print("WORST cosine %s %s" % (kind, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("n,n_sel,d", lb.SHAPES, ids=["%dof%dx%d" % (s[1], s[0], s[2]) for s in lb.SHAPES])
def test_l1_loss_within_its_limit_and_gradient_bit_by_bit(n, n_sel, d):
    """(lb.ratios compares the L1 gradient with sign(fp32 difference) * s32 bit by bit: +0 where a == b and outside sel)"""
    cs = lb.case("gauss", n, n_sel, d, "l1")
    worst = {}
    _check(Run(cs.out, cs.sel, cs.target, "l1"), cs, "l1 gauss %d of %d x %d" % (n_sel, n, d), worst)
    assert worst["grad"] == 0 and worst["zeros"] == 0
    print("WORST l1 gauss %s" % "  ".join("%s %.3f" % kv for kv in sorted(worst.items())))


def test_a_sorted_selection_gives_the_same_rows():
    """The one sorted case; and the same (row, target) pairs handed over in sorted order give every gradient row bit by bit."""
    kind, n, n_sel, d = lb.SORTED_CASE
    cs = lb.case(kind, n, n_sel, d, sort=True)
    _check(Run(cs.out, cs.sel, cs.target, "cosine"), cs, "cosine %s sorted" % kind, {})
    cu = lb.case(kind, n, n_sel, d)
    order = np.argsort(cu.sel)
    for loss_type in lb.LOSS_TYPES:
        g_unsorted, _ = Run(cu.out, cu.sel, cu.target, loss_type).backward(2.5)
        g_sorted, _ = Run(cu.out, cu.sel[order], cu.target[order], loss_type).backward(2.5)
        assert _same_bits(g_unsorted, g_sorted), loss_type


REPEAT = [("aligned", 50, 37, 768), ("gauss", 2052, 2049, 20), ("clamp", 1023, 1023, 20)]


@pytest.mark.parametrize("loss_type", lb.LOSS_TYPES)
@pytest.mark.parametrize("kind,n,n_sel,d", REPEAT, ids=["%s-%dof%dx%d" % (k, s, n, d) for (k, n, s, d) in REPEAT])
def test_loss_and_gradient_are_repeatable_bit_by_bit(kind, n, n_sel, d, loss_type):
    cs = lb.case(kind if loss_type == "cosine" else "gauss", n, n_sel, d, loss_type)
    one, two = Run(cs.out, cs.sel, cs.target, loss_type), Run(cs.out, cs.sel, cs.target, loss_type)
    assert _same_bits(one.loss.reshape(1), two.loss.reshape(1))
    g1 = one.backward(2.5)[0].clone()
    g2 = one.backward(2.5)[0]                                # a second backward pass from the same forward pass
    assert g1.data_ptr() != g2.data_ptr() and _same_bits(g1, g2)
    assert _same_bits(g1, two.backward(2.5)[0])


HINTS = [("gauss", 50, 37, 260), ("aligned", 50, 37, 4), ("clamp", 2052, 2049, 20), ("gauss", 6, 4, 20)]


@pytest.mark.parametrize("loss_type", lb.LOSS_TYPES)
@pytest.mark.parametrize("kind,n,n_sel,d", HINTS, ids=["%s-%dof%dx%d" % (k, s, n, d) for (k, n, s, d) in HINTS])
def test_compacted_rows_and_inverse_table_describe_the_dense_gradient(kind, n, n_sel, d, loss_type):
    """What the network executor's row-sparse head reads: rows[j] is bitwise the dense gradient row idx[j], and the first n int32 of
    the state are the inverse of sel (-1 elsewhere) -- for an UNSORTED sel."""
    cs = lb.case(kind if loss_type == "cosine" else "gauss", n, n_sel, d, loss_type)
    assert (np.diff(cs.sel) < 0).any()
    run = Run(cs.out, cs.sel, cs.target, loss_type)
    g, hint = run.backward(-0.75)
    assert hint is not None and hint["ptr"] == g.data_ptr() and hint["shape"] == (n, d) and hint["version"] == g._version
    assert torch.equal(hint["idx"], run.sel) and hint["rows"].shape == (n_sel, d)
    assert _same_bits(hint["rows"], g.index_select(0, hint["idx"]))
    assert hint["pos_ptr"] == hint["state"].data_ptr()
    pos = hint["state"][:4 * n].view(torch.int32).cpu().numpy()
    want = np.full(n, -1, dtype=np.int32)
    want[cs.sel] = np.arange(n_sel, dtype=np.int32)
    assert np.array_equal(pos, want)


@pytest.mark.parametrize("loss_type", lb.LOSS_TYPES)
def test_no_hint_when_every_row_is_selected(loss_type):
    cs = lb.case("gauss", 1023, 1023, 20, loss_type)
    g, hint = Run(cs.out, cs.sel, cs.target, loss_type).backward()
    assert hint is None and not hasattr(g, "_osn_rows")


def test_clamp_rows_have_their_closed_forms():
    """A zero output row gives -up / n_sel * b / (eps nb) (within its limit, which _check holds it to: here the closed form itself to
    2 (q + 7) u, the T1 path alone); a zero target row and a row pair of zeros give +-0."""
    cs = lb.case("clamp", 50, 37, 516)
    r = lb.reference(cs.out, cs.sel, cs.target, "cosine", 2.5)
    g = Run(cs.out, cs.sel, cs.target, "cosine").backward(2.5)[0].cpu().numpy()
    assert np.isfinite(g).all()
    a_zero, b_zero = ~cs.out[cs.sel].any(axis=1), ~cs.target.any(axis=1)
    assert (a_zero & ~b_zero).any() and (b_zero & ~a_zero).any() and (a_zero & b_zero).any()
    for j in np.flatnonzero(a_zero & ~b_zero):
        b = cs.target[j].astype(np.float64)
        want = -2.5 / 37 * b / (1e-8 * max(np.sqrt(r.B[j]), 1e-8))
        assert (np.abs(g[cs.sel[j]] - want) <= 2 * (lb.q_of(516) + 7) * lb.U * np.abs(want) + lb.FLOOR).all()
    assert not g[cs.sel[b_zero]].any()


def _rows_but(t, r):
    keep = torch.ones(t.shape[0], dtype=torch.bool, device=t.device)
    keep[r] = False
    return t[keep]


NONFINITE = [(50, 37, 260), (2052, 2049, 20)]


@pytest.mark.parametrize("n,n_sel,d", NONFINITE, ids=["%dof%dx%d" % (s[1], s[0], s[2]) for s in NONFINITE])
@pytest.mark.parametrize("where", ["output nan", "output inf", "target nan"])
def test_cosine_a_non_finite_value_stays_in_its_row(n, n_sel, d, where):
    """NaN or +inf at one element of a selected output row, or NaN in a target row: the loss is not finite, that row of the gradient is
    NaN in EVERY element (as torch's: the row's norm is not finite), and every other row keeps its bits."""
    cs = lb.case("gauss", n, n_sel, d)
    out, sel, target = _t(cs.out), _t(cs.sel), _t(cs.target)
    clean_run = Run(out, sel, target, "cosine")
    clean = clean_run.backward(2.5)[0].clone()
    assert bool(torch.isfinite(clean).all()) and bool(torch.isfinite(clean_run.loss))
    j = n_sel - 2
    r = int(cs.sel[j])
    if where.startswith("output"):
        out = out.clone()
        out[r, d - 3] = float("nan") if where.endswith("nan") else float("inf")
    else:
        target = target.clone()
        target[j, d - 3] = float("nan")
    run = Run(out, sel, target, "cosine")
    g, hint = run.backward(2.5)
    assert not bool(torch.isfinite(run.loss)), "loss %r" % run.loss.item()
    assert bool(torch.isnan(g[r]).all()), "%d of %d elements of the row are not NaN" % (int((~torch.isnan(g[r])).sum()), d)
    assert _same_bits(_rows_but(g, r), _rows_but(clean, r))
    assert bool(torch.isnan(hint["rows"][j]).all()) and _same_bits(_rows_but(hint["rows"], j), _rows_but(clean.index_select(0, sel), j))


@pytest.mark.parametrize("loss_type", lb.LOSS_TYPES)
def test_a_nan_outside_the_selection_changes_nothing(loss_type):
    cs = lb.case("gauss", 50, 37, 260, loss_type)
    outside = np.flatnonzero(~np.isin(np.arange(cs.n), cs.sel))
    out = _t(cs.out)
    clean_run = Run(out, cs.sel, cs.target, loss_type)
    clean = clean_run.backward(2.5)[0].clone()
    out2 = out.clone()
    out2[int(outside[0])] = float("nan")
    out2[int(outside[-1]), 7] = float("inf")
    run = Run(out2, cs.sel, cs.target, loss_type)
    assert _same_bits(run.loss.reshape(1), clean_run.loss.reshape(1)) and _same_bits(run.backward(2.5)[0], clean)


@pytest.mark.parametrize("n,n_sel,d", NONFINITE, ids=["%dof%dx%d" % (s[1], s[0], s[2]) for s in NONFINITE])
def test_l1_non_finite_elements(n, n_sel, d):
    """L1: a NaN element makes the loss NaN and has the gradient 0 (torch.sign of NaN has gradient 0 as well); a +inf element makes
    the loss +inf and has the gradient +s32 (-s32 in the target); every other element keeps its bits."""
    cs = lb.case("gauss", n, n_sel, d, "l1")
    out, sel, target = _t(cs.out), _t(cs.sel), _t(cs.target)
    clean = Run(out, sel, target, "l1").backward(2.5)[0].clone()
    s32 = float(lb.reference(cs.out, cs.sel, cs.target, "l1", 2.5).s32)
    j = n_sel - 2
    r, c = int(cs.sel[j]), d - 3
    for value, in_target, want_loss, want in ((float("nan"), False, "nan", 0.0), (float("nan"), True, "nan", 0.0),
                                              (float("inf"), False, "inf", s32), (float("inf"), True, "inf", -s32)):
        o, t = out.clone(), target.clone()
        if in_target:
            t[j, c] = value
        else:
            o[r, c] = value
        run = Run(o, sel, t, "l1")
        g = run.backward(2.5)[0].clone()
        loss = run.loss.item()
        assert (loss != loss) if want_loss == "nan" else (loss == float("inf")), loss
        expect = clean.clone()
        expect[r, c] = want
        assert _same_bits(g, expect), "value %r in the %s: gradient element %r" % (value, "target" if in_target else "output", g[r, c].item())
