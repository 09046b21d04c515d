"""What gives tests/test_gpu_loss_bounds.py its teeth, checked without a GPU: on every shape and input kind the GPU module uses, the
numpy emulation of the loss kernels' arithmetic (loss_bounds.emulate) meets every limit of loss_bounds with a worst ratio <= 0.5, the
margin the limits have over correct arithmetic; the same emulation with ONE defect (loss_bounds.MUTANTS) breaks a limit; the
reference agrees with oracle/loss.py (pinned to torch's autograd) to 1e-12; and the inputs are what their names say.

Worst err / limit of the correct emulation over all cases: cosine gradient 0.194, cosine loss 0.020, L1 loss 0.073; the gradient limit
is the split one of loss_bounds (common / T1 / T2 roundings), never above the single-constant form C_g u |s| (|b_i| + (S / A) |a_i|) / (na nb).

What the criteria of test_gpu_dense.py::test_distill_loss_forward_and_gradient (gradient rows within 2e-6 of the row's largest element,
loss within 1e-6) make of each mutant on that test's own three shapes, Gaussian rows and sorted selection (measured, asserted below):
    a  ka scaled by (1 + 3e-6)                     passes them; breaks the gradient limit on aligned rows at d = 4 (1.4) and d = 20 (1.1).
                                                   At d >= 252 the doubled rounding count 2 (2 q + 11) reaches 3e-6 / u = 50 and the
                                                   limit can no longer tell this defect from rounding: it is seen at the narrow widths only
    b  ka without its `sqrtf(a2) > eps` test       passes them (no row near the clamp); breaks the gradient limit on the clamp rows
    c  norms not clamped in the gradient           passes them;                         inf / NaN on the zero rows here
    d  target row by rank, not by pos[r]           passes them (every selection sorted); breaks the gradient limit on every case here
    f  last partial 256-column step dropped        passes them (768, 512 and 20 have none); breaks gradient and loss at 260, 516, 1028
    h  L1: +s at a == b                            passes them (no equal elements);     breaks the bit-by-bit L1 gradient
    e  butterfly started at 16                     caught there (d = 768, 512) and here
    g  mean without the rows from 1024 k on        passes the gradient criterion, caught by the loss criterion at n_sel = 1200; here at
                                                   1025 and 2049
The other way round: on ALIGNED rows (a = t b + noise, relative noise 1e-5 .. 1e-1) the correct emulation is 3.0e3 (d = 4) to 1.1e4
(d = 256) times beyond "2e-6 of the row's largest element" -- the two terms of the gradient cancel, the row's largest element is the
small difference -- so that criterion cannot be applied in the regime training moves into; the limits here hold there at <= 0.16.
"""
import functools

import numpy as np
import pytest

import loss_bounds as lb
from oracle import loss as ol

MARGIN = 0.5
CASES = [(k, n, n_sel, d) for k in lb.KINDS for (n, n_sel, d) in lb.SHAPES]
IDS = ["%s-%dof%dx%d" % (k, n_sel, n, d) for (k, n, n_sel, d) in CASES]
# where each mutant is looked for (kind, n, n_sel, d, loss type): the kinds and shapes at which it acts
MUTANT_CASES = [("aligned", 50, 37, 4, "cosine"), ("aligned", 50, 37, 20, "cosine"), ("aligned", 50, 37, 768, "cosine"),
                ("gauss", 50, 37, 260, "cosine"), ("gauss", 50, 37, 1028, "cosine"), ("clamp", 50, 37, 516, "cosine"),
                ("gauss", 1027, 1025, 20, "cosine"), ("gauss", 2052, 2049, 20, "cosine"), ("gauss", 50, 37, 260, "l1"),
                ("gauss", 1027, 1025, 20, "l1")]
# the criteria of test_gpu_dense.py on its own three shapes and Gaussian rows let these mutants pass (gradient AND loss criterion)
PASS_THE_DENSE_CHECK = ("a", "b", "c", "d", "f", "h")


def _all_ups(cs, mutant=None):
    for up in lb.UPS:
        r = lb.reference(cs.out, cs.sel, cs.target, cs.loss_type, up)
        yield up, r, lb.limits(r), lb.emulate(cs.out, cs.sel, cs.target, cs.loss_type, up, mutant=mutant)


@pytest.mark.parametrize("kind,n,n_sel,d", CASES, ids=IDS)
def test_the_emulation_meets_every_limit_with_margin(kind, n, n_sel, d):
    cs = lb.case(kind, n, n_sel, d)
    for up, r, L, got in _all_ups(cs):
        label = "%s %d of %d x %d up %g" % (kind, n_sel, n, d, up)
        flat = lb.within(got, r, L, label)
        print("RATIO %s %s" % (label, "  ".join("%s %.3f" % kv for kv in sorted(flat.items()))))
        for name, ratio in flat.items():
            assert ratio <= MARGIN, "%s: %s at %.3f of its limit: the derivation misses a term" % (label, name, ratio)
        # the split limit never exceeds the single-constant form C_g u |s| (|b_i| + (S / A) |a_i|) / (na nb)
        assert (L.grad[cs.sel] <= lb.limit_single(r) * (1 + 1e-12)).all()
        if kind == "clamp":
            assert np.isfinite(got["grad"]).all() and np.isfinite(r.grad).all()


L1_CASES = [("gauss", n, n_sel, d) for (n, n_sel, d) in lb.SHAPES]


@pytest.mark.parametrize("kind,n,n_sel,d", L1_CASES, ids=["l1-%dof%dx%d" % (n_sel, n, d) for (_, n, n_sel, d) in L1_CASES])
def test_the_l1_emulation_meets_its_limit_and_the_gradient_bit_by_bit(kind, n, n_sel, d):
    cs = lb.case(kind, n, n_sel, d, "l1")
    assert 0.05 < float((cs.out[cs.sel] == cs.target).mean()) < 0.2 or n_sel * d < 1000
    for up, r, L, got in _all_ups(cs):
        flat = lb.within(got, r, L, "l1 %d of %d x %d up %g" % (n_sel, n, d, up))
        assert flat["loss"] <= MARGIN and flat["grad"] == 0 and flat["zeros"] == 0
        assert np.array_equal(np.sign(r.grad32.astype(np.float64)), np.sign(r.grad))                      # fp32 and fp64 signs agree


def test_the_sorted_selection_is_a_case_too():
    kind, n, n_sel, d = lb.SORTED_CASE
    cs = lb.case(kind, n, n_sel, d, sort=True)
    assert (np.diff(cs.sel) > 0).all()
    for up, r, L, got in _all_ups(cs):
        assert max(lb.within(got, r, L, "sorted").values()) <= MARGIN


@pytest.mark.parametrize("loss_type", lb.LOSS_TYPES)
def test_the_reference_agrees_with_the_oracle(loss_type):
    for (n, n_sel, d) in [(50, 37, 260), (1027, 1025, 20), (50, 37, 4)]:
        cs = lb.case("gauss", n, n_sel, d, loss_type)
        r = lb.reference(cs.out, cs.sel, cs.target, loss_type, 1.0)
        loss, grad = ol.distill_loss(cs.out, cs.sel, cs.target, loss_type)
        assert abs(r.loss - loss) <= 1e-12 * abs(loss)
        scale = np.abs(grad).max(axis=1, keepdims=True)
        assert (np.abs(r.grad - grad) <= 1e-12 * scale).all() and not r.grad[~r.keep].any()


def test_input_kinds_are_what_their_names_say():
    for d in (4, 20, 768):
        cs = lb.case("aligned", 50, 37, d)
        r = lb.reference(cs.out, cs.sel, cs.target)
        a, b = cs.out[cs.sel].astype(np.float64), cs.target.astype(np.float64)
        exact = np.arange(37) % 10 == 0
        t = (a[:, 0] / b[:, 0])[exact]
        assert np.array_equal(a[exact], t[:, None] * b[exact]) and (t < 0).any() and (t > 0).any()
        pos = exact & (a[:, 0] / b[:, 0] > 0)
        assert (r.val[pos] < 1e-8).all() and (np.abs(r.val[exact & ~pos] - 2) < 1e-8).all()             # 1 - cos < 1e-8 is reached
        if d >= 20:
            assert r.val[~exact].min() < 1e-6 and r.val[~exact].max() > 1e-4                            # and the way there is covered
    cs = lb.case("decades", 50, 37, 768)
    sd = cs.out[cs.sel].astype(np.float64).std(0)
    assert sd.max() / sd.min() > 1e4
    cs = lb.case("clamp", 50, 37, 516)
    r = lb.reference(cs.out, cs.sel, cs.target)
    za, zb = r.A == 0, r.B == 0
    assert (za & ~zb).any() and (zb & ~za).any() and (za & zb).any()
    assert ((r.A > 0) & ~r.live).any() and (r.live & (np.sqrt(r.A) < 3e-8)).any()
    assert ((r.B > 0) & (np.sqrt(r.B) < 1e-8)).any() and ((np.sqrt(r.B) > 1e-8) & (np.sqrt(r.B) < 3e-8)).any()
    assert not cs.out.flags.writeable and not cs.target.flags.writeable
    # a zero output row: -up / n_sel * b / (1e-8 nb); a zero target row: a zero gradient
    j = int(np.flatnonzero(za & ~zb)[0])
    want = -1.0 / 37 * cs.target[j].astype(np.float64) / (1e-8 * max(np.sqrt(r.B[j]), 1e-8))
    assert np.allclose(r.grows[j], want, rtol=1e-12, atol=0)
    assert not r.grows[zb].any()
    for (n, n_sel, d) in lb.SHAPES:                                     # (rows() asserts the input conditions as it makes them)
        for kind in lb.KINDS:
            lb.case(kind, n, n_sel, d)
    assert [s[0] - s[1] for s in lb.N_SHAPES] == [0, 1, 2, 3, 0, 1, 2, 3]


@functools.lru_cache(maxsize=None)
def _dense(n, n_sel, d, loss_type):
    out, sel, target = lb.dense_inputs(n, n_sel, d, loss_type)
    loss, grad = ol.distill_loss(out, sel, target, loss_type)
    return out, sel, target, loss, grad


def _dense_verdict(mutant, loss_type):
    """(every shape passes the gradient criterion, every shape passes gradient and loss criterion) of test_gpu_dense.py."""
    res = [lb.dense_check(lb.emulate(out, sel, target, loss_type, 2.5, mutant=mutant), loss, grad, 2.5)
           for out, sel, target, loss, grad in (_dense(*s, loss_type) for s in lb.DENSE_SHAPES)]
    return all(g for g, _ in res), all(g and l for g, l in res)


@pytest.mark.parametrize("mutant", lb.MUTANTS)
def test_each_mutant_breaks_a_limit(mutant):
    broke = []
    for key in MUTANT_CASES:
        if (key[4] == "l1") != (mutant in "h") and mutant not in "efg":
            continue
        cs = lb.case(*key)
        for up, r, L, got in _all_ups(cs, mutant):
            res = lb.ratios(got, r, L)
            bad = sorted(k for k, v in res.items() if v[1])
            if bad:
                broke.append((key, up))
                print("mutant %s %s up %g: beyond the limit: %s" % (mutant, key, up, {k: "%.3g" % res[k][0] for k in bad}))
    grad_ok, all_ok = _dense_verdict(mutant, "l1" if mutant == "h" else "cosine")
    print("mutant %s: test_gpu_dense.py's gradient criterion %s, gradient and loss criteria %s"
          % (mutant, "pass" if grad_ok else "fail", "pass" if all_ok else "fail"))
    assert broke, "mutant %s stays inside every limit on every case" % mutant
    # the gap on record: these defects pass test_gpu_dense.py's criteria on its own shapes and inputs
    assert all_ok == (mutant in PASS_THE_DENSE_CHECK), "mutant %s: the older criteria %s it" % (mutant, "pass" if all_ok else "catch")


def test_the_correct_emulation_passes_the_older_criteria_on_their_inputs_and_not_on_aligned_rows():
    """On its own Gaussian rows the 2e-6-of-the-row-maximum criterion passes the correct arithmetic (so a mutant failing it above is
    the mutant's doing); on aligned rows the SAME correct arithmetic is far beyond it -- the criterion cannot be applied in the
    regime training moves into, the limits of loss_bounds can."""
    for loss_type in lb.LOSS_TYPES:
        assert _dense_verdict(None, loss_type) == (True, True)
    factor = 0.0
    for (n, n_sel, d) in lb.D_SHAPES:
        cs = lb.case("aligned", n, n_sel, d)
        r = lb.reference(cs.out, cs.sel, cs.target)
        got = lb.emulate(cs.out, cs.sel, cs.target)
        lb.within(got, r, lb.limits(r), "aligned x %d" % d)
        noisy = np.arange(n_sel) % 10 != 0                               # (a = +-t b exactly: the exact gradient is 0, any error is "infinitely" beyond)
        err = np.abs(got["grad"][cs.sel].astype(np.float64) - r.grows)[noisy]
        scale = np.abs(r.grows).max(axis=1, keepdims=True)[noisy]
        with np.errstate(divide="ignore", invalid="ignore"):
            f = float(np.nanmax(np.where(err > 0, err / (2e-6 * scale + 1e-30), 0.0)))
        print("aligned x %d: correct fp32 arithmetic at %.3g of the 2e-6-of-the-row-maximum criterion" % (d, f))
        factor = max(factor, f)
    assert factor > 100, factor
