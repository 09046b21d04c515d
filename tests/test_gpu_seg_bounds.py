"""The supervised head on the MI355X (csrc/seg.hip through losses.segmentation_loss and ops.seg_* only; osn_sgd_step / osn_adam_step of
csrc/optim.hip called directly) against the per-row and per-element limits of tests/seg_bounds.py, at the edges of the kernels' own
loops -- every class-count bucket (c = 8|9 .. 128|129), the confusion histogram's switch from LDS to global atomics (c = 90|91), the
first second trip of the grid-stride loops (n = 512 RPI + 1) and seg_mean_kernel's strided read of more than 256 partials -- on
Gaussian, confident, +-1e4, tied and wide rows, at three upstream gradients.  test_seg_bounds_cpu.py shows that these limits separate
the kernels' arithmetic (ratio <= 0.5) from nine single defects, three of which the criteria of test_gpu_seg.py let pass.

Also: the loss of single rows; the gathered forward; the confusion matrix; bitwise repeatability; the test-repeat vote bit by bit; rows
with non-finite logits; two finite cases bit by bit against outputs recorded from the build before the non-finite fix; and one
optimizer step against the update rule in float64.

Worst err / limit per kind and quantity, measured on an MI355X (the "RATIO" lines, all shapes and upstream gradients; the numpy
emulation of test_seg_bounds_cpu.py in brackets -- its exp and log1p are correctly rounded, the device's are 0.85 and 0.56 ulp off
at worst, tools/probe_libm.hip):
    gauss      gradient 0.401 (0.401)   loss 0.220 (0.220)
    confident  gradient 0.445 (0.445)   loss 0.171 (0.171)   single rows 0.265 (c = 2), 0.148 (20), 0.158 (160), the smallest 2e-63
    big        gradient 0.348 (0.348)   loss 0.161 (0.161)
    ties       gradient 0.345 (0.368)   loss 0.087 (0.087)
    wide       gradient 0.446 (0.446)   loss 0.178 (0.178)   single rows 0.301 (c = 2), 0.323 (20), 0.257 (160)
    gathered forward: loss 0.101;  a -inf logit off the label: gradient 0.359, loss 0.093;  rows without a valid label: +0 in every case
    one SGD step: 0.500 in every setting (p - lr d is one rounding of |p'| plus one of |lr d|: half of the doubled count);
    one Adam step: parameters 0.500, first moments 0.498, second moments 0.499

FOUND with the first run of test_a_nan_or_an_overflowed_logit_poisons_its_row_and_no_other, as reading the kernel had suggested: a row
with one +inf logit has m = +inf and, the argmax being kept out of the sum, s1 = 0 and inv = 1.  With the label off the argmax the loss
was +inf (not NaN) and the row's gradient the finite sc * (1 at the argmax, -1 at the label, 0 elsewhere); with the label on the argmax
the loss was NaN but the row's gradient all zeros (-0 at the argmax) -- a finite gradient from an overflowed logit, where float64 torch
has NaN in every element.  A NaN logit and a row of -inf already behaved as torch (c >= 2).  csrc/seg.hip now sets s1 to NaN when the
row maximum is not finite, which makes loss and row NaN in all these cases (and for c = 1).  Every finite row keeps its bits: two cases
are compared bit by bit with loss and gradient recorded from the build BEFORE that change (tests/golden/seg_parent_bits.npz, recorded on
an MI355X by running these very inputs through the parent commit's library), not merely shown in the emulation.  Nothing else was found:
every limit, the confusion matrix, the votes and both optimizer steps held on the first run.
"""
import functools
import os

import numpy as np
import pytest
import torch

import seg_bounds as sb

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


def dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.array(a)).to(dev())                # (a copy: the shared inputs are read-only)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class Run:
    """One forward pass of segmentation_loss on device copies of (x, y); backward(up) -> the gradient of (loss * up)."""

    def __init__(self, x, y, ignore):
        from openscene_amd.losses import segmentation_loss
        self.x = (x if torch.is_tensor(x) else _t(x)).clone().requires_grad_(True)
        self.y = y if torch.is_tensor(y) else _t(y)
        self.loss = segmentation_loss(self.x, self.y, ignore_index=ignore)

    def backward(self, up=1.0):
        self.x.grad = None
        (self.loss * up).backward(retain_graph=True)
        return self.x.grad


def _check(cs, label, worst):
    run = Run(cs.x, cs.y, cs.ignore)
    loss = run.loss.item()
    for up in sb.UPS:
        r = sb.reference(cs.x, cs.y, cs.ignore, up)
        g = run.backward(up).cpu().numpy()
        flat = sb.within({"loss": np.float32(loss), "grad": g}, r, sb.limits(r), "%s up %g" % (label, up), worst)
        print("RATIO %s up %g %s" % (label, up, "  ".join("%s %.3f" % kv for kv in sorted(flat.items()))))


C_CASES = [(k, n, c) for (n, c) in sb.C_SHAPES for k in sb.KINDS]
N_CASES = [(k, n, c) for (n, c) in sb.N_SHAPES for k in sb.N_KINDS]


@pytest.mark.parametrize("kind,n,c", C_CASES + N_CASES, ids=["%s-%dx%d" % k for k in C_CASES + N_CASES])
def test_loss_and_gradient_within_the_limits(kind, n, c):
    worst = {}
    _check(sb.case(kind, n, c), "%s %d x %d" % (kind, n, c), worst)
    print("WORST %s %s" % (kind, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("c", [2, 20, 160])
@pytest.mark.parametrize("kind", ["confident", "wide"])
def test_the_loss_of_each_single_row(kind, c):
    """Every other label ignored: the returned scalar is that row's val exactly (one term, n_valid = 1), held to the row's own limit --
    a confident row keeps its small loss (log1pf, not logf(1 + s1))."""
    from openscene_amd.losses import segmentation_loss
    cs = sb.case(kind, sb.C_ROWS, c)
    r = sb.reference(cs.x, cs.y, cs.ignore)
    L = sb.limits(r)
    x = _t(cs.x)
    js = np.flatnonzero(r.valid)
    got = torch.empty(len(js), device=dev())
    for i, j in enumerate(js):
        y = np.full(cs.n, cs.ignore, dtype=np.int64)
        y[j] = cs.y[j]
        got[i] = segmentation_loss(x, _t(y), ignore_index=cs.ignore)
    err = np.abs(got.cpu().numpy().astype(np.float64) - r.val[js])
    ratio, bad = sb._worst(err, L.val[js])
    print("RATIO rows %s x %d val %.3f  (smallest row loss %.3g)" % (kind, c, ratio, r.val[js].min()))
    assert not bad, "%d row losses beyond the limit, worst %.3g" % (bad, ratio)


@pytest.mark.parametrize("kind,n,c", [(k, n, c) for (n, c) in sb.C_SHAPES for k in ("gauss", "ties")],
                         ids=["%s-%dx%d" % (k, n, c) for (n, c) in sb.C_SHAPES for k in ("gauss", "ties")])
def test_gathered_forward(kind, n, c):
    """rows= with duplicates, unsorted, under no_grad: the loss of logits[rows] within its limit, pred exact."""
    from openscene_amd.losses import segmentation_loss
    cs = sb.case(kind, n, c)
    g = np.random.default_rng(sb._seed("gather", kind, n, c))
    rows = np.concatenate([g.permutation(n), g.integers(0, n, 2 * n)])
    rows = rows[g.permutation(3 * n)].astype(np.int64)
    y = np.where(g.random(3 * n) < 0.15, cs.ignore, g.integers(0, c, 3 * n)).astype(np.int64)
    assert (np.diff(rows) < 0).any() and len(np.unique(rows)) < len(rows)
    with torch.no_grad():
        loss, pred = segmentation_loss(_t(cs.x), _t(y), ignore_index=cs.ignore, rows=_t(rows), pred=True, validate=True)
    r = sb.reference(cs.x[rows], y, cs.ignore)
    flat = sb.within({"loss": np.float32(loss.item())}, r, sb.limits(r), "gathered %s %d x %d" % (kind, n, c))
    print("RATIO gathered %s %d x %d loss %.3f" % (kind, n, c, flat["loss"]))
    assert np.array_equal(pred.cpu().numpy(), r.pred)


@pytest.mark.parametrize("c", [89, 90, 91, 256])
def test_confusion_matrix_is_exact(c):
    """Both sides of the LDS / global-atomics switch and the widest head, tied rows, two calls into one matrix (the second gathered),
    n_lab past the first trip of the grid-stride loop."""
    from openscene_amd import ops
    rpi = sb.SEG_THREADS // sb.seg_group(c)
    n = sb.SEG_MAX_WG * rpi + 5
    ign = sb.ignore_of(c)
    g = np.random.default_rng(sb._seed("conf", c))
    x, y = sb.rows("ties", n, c, g)
    assert sb.seg_grid(n, c) == sb.SEG_MAX_WG and n > sb.SEG_MAX_WG * rpi
    conf = torch.zeros(c, c, dtype=torch.int64, device=dev())
    xd = _t(x)
    _, pred, _ = ops.seg_loss_fwd(xd, _t(y), ign, want_pred=True, confusion=conf, validate=True)
    ref_pred = np.argmax(x, axis=1)
    assert np.array_equal(pred.cpu().numpy(), ref_pred)
    want = np.bincount((ref_pred * c + y)[y != ign], minlength=c * c).reshape(c, c)
    assert np.array_equal(conf.cpu().numpy(), want)
    rows = g.integers(0, n, n + 11).astype(np.int64)
    y2 = np.where(g.random(n + 11) < 0.15, ign, g.integers(0, c, n + 11)).astype(np.int64)
    _, pred2, _ = ops.seg_loss_fwd(xd, _t(y2), ign, rows=_t(rows), want_loss=False, want_pred=True, confusion=conf, validate=True)
    assert np.array_equal(pred2.cpu().numpy(), ref_pred[rows])
    want = want + np.bincount((ref_pred[rows] * c + y2)[y2 != ign], minlength=c * c).reshape(c, c)
    assert np.array_equal(conf.cpu().numpy(), want) and int(want.sum()) == int((y != ign).sum() + (y2 != ign).sum())


@pytest.mark.parametrize("c", [8, 16, 20, 64, 128, 129])
def test_loss_and_gradient_are_repeatable_bit_by_bit(c):
    """One case per group size, past the first trip of the grid-stride loop."""
    n = sb.SEG_MAX_WG * (sb.SEG_THREADS // sb.seg_group(c)) + 3
    g = np.random.default_rng(sb._seed("repeat", c))
    x, y = sb.rows("gauss", n, c, g)
    x, y = _t(x), _t(y)
    one, two = Run(x, y, 255), Run(x, y, 255)
    assert _same_bits(one.loss.reshape(1), two.loss.reshape(1))
    g1 = one.backward(2.5).clone()
    g2 = one.backward(2.5)                                    # a second backward pass from the same forward pass
    assert g1.data_ptr() != g2.data_ptr() and _same_bits(g1, g2)
    assert _same_bits(g1, two.backward(2.5))


@pytest.mark.parametrize("kind,n,c", sb.PARENT_CASES, ids=["%s-%dx%d" % k for k in sb.PARENT_CASES])
def test_finite_rows_keep_the_bits_of_the_build_before_the_non_finite_fix(kind, n, c):
    """tests/golden/seg_parent_bits.npz: loss and gradient (up = 2.5) of these cases as the kernels gave them before seg.hip learnt to
    poison s1 on a non-finite row maximum, recorded on an MI355X with the same compiler."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seg_parent_bits.npz"))
    cs = sb.case(kind, n, c)
    run = Run(cs.x, cs.y, cs.ignore)
    key = "%s_%d_%d" % (kind, n, c)
    assert np.array_equal(run.loss.detach().reshape(1).cpu().numpy().view(np.int32), z[key + "_loss"])
    assert np.array_equal(run.backward(2.5).cpu().numpy().view(np.int32), z[key + "_grad"])


# ------------------------------------------------------------------------------------------------ non-finite logits
NF_SHAPES = [(37, 2), (37, 20), (300, 129)]


def _nf_setup(n, c):
    cs = sb.case("gauss", n, c)
    y = np.array(cs.y)
    j = int(np.flatnonzero(y != cs.ignore)[len(y) // 3])      # a labelled row in the middle
    ig = int(np.flatnonzero(y == cs.ignore)[0])               # an ignored row
    return cs, y, j, ig


def _rows_but(t, j):
    keep = torch.ones(t.shape[0], dtype=torch.bool, device=t.device)
    keep[j] = False
    return t[keep]


@pytest.mark.parametrize("n,c", NF_SHAPES, ids=["%dx%d" % s for s in NF_SHAPES])
@pytest.mark.parametrize("label", ["on", "off"])
@pytest.mark.parametrize("what", ["nan", "inf", "all -inf"])
def test_a_nan_or_an_overflowed_logit_poisons_its_row_and_no_other(n, c, what, label):
    """A NaN or a +inf at one element of a labelled row (the label on that column, the row's argmax, or off it), or a row of -inf:
    the loss is NaN and that row of the gradient is NaN in EVERY element, as float64 torch has it; every other row keeps its bits."""
    cs, y, j, _ = _nf_setup(n, c)
    k = c - 1
    y[j] = k if label == "on" else k - 1
    clean = Run(cs.x, y, cs.ignore)
    gc = clean.backward(2.5).clone()
    assert bool(torch.isfinite(gc).all()) and bool(torch.isfinite(clean.loss))
    x = _t(cs.x)
    if what == "all -inf":
        x[j] = -INF
    else:
        x[j, k] = NAN if what == "nan" else INF
    run = Run(x, y, cs.ignore)
    g = run.backward(2.5)
    # float64 torch on the same values
    xd = x.detach().cpu().double().requires_grad_()
    ref = torch.nn.functional.cross_entropy(xd, torch.from_numpy(y), ignore_index=cs.ignore)
    (ref * 2.5).backward()
    assert bool(torch.isnan(ref)) and bool(torch.isnan(xd.grad[j]).all())
    assert bool(torch.isnan(run.loss)), "loss %r" % run.loss.item()
    assert bool(torch.isnan(g[j]).all()), "%d of %d elements of the row are not NaN: %r" % (int((~torch.isnan(g[j])).sum()), c, g[j].tolist()[:8])
    assert _same_bits(_rows_but(g, j), _rows_but(gc, j))


@pytest.mark.parametrize("n,c", NF_SHAPES, ids=["%dx%d" % s for s in NF_SHAPES])
def test_minus_infinity_at_one_column(n, c):
    """-inf at a column that is not the label: loss and row finite and within the limits, +-0 at that column.  -inf at the label:
    the loss is +inf, the row's gradient finite with -s at the label.  Every other row keeps its bits."""
    cs, y, j, _ = _nf_setup(n, c)
    lab = int(y[j])
    k = (lab + 1) % c
    clean = Run(cs.x, y, cs.ignore)
    gc = clean.backward(2.5).clone()
    x = np.array(cs.x)
    x[j, k] = -INF
    run = Run(x, y, cs.ignore)
    g = run.backward(2.5)
    r = sb.reference(x, y, cs.ignore, 2.5)
    flat = sb.within({"loss": np.float32(run.loss.item()), "grad": g.cpu().numpy()}, r, sb.limits(r), "-inf off the label %d x %d" % (n, c))
    print("RATIO -inf off the label %d x %d %s" % (n, c, flat))
    assert g[j, k].item() == 0.0 and bool(torch.isfinite(g[j]).all()) and bool(torch.isfinite(run.loss))
    assert _same_bits(_rows_but(g, j), _rows_but(gc, j))
    x = np.array(cs.x)
    x[j, lab] = -INF
    run = Run(x, y, cs.ignore)
    g = run.backward(2.5)
    r = sb.reference(x, y, cs.ignore, 2.5)
    assert run.loss.item() == INF
    res = sb.ratios({"grad": g.cpu().numpy()}, r, sb.limits(r))
    assert not res["grad"][1] and not res["zeros"][1], res
    s32 = np.float32(2.5) / np.float32(r.n_valid)
    assert bool(torch.isfinite(g[j]).all()) and g[j, lab].item() == -float(s32)
    assert _same_bits(_rows_but(g, j), _rows_but(gc, j))


@pytest.mark.parametrize("n,c", NF_SHAPES, ids=["%dx%d" % s for s in NF_SHAPES])
def test_non_finite_values_in_an_ignored_row_change_nothing(n, c):
    cs, y, j, ig = _nf_setup(n, c)
    clean = Run(cs.x, y, cs.ignore)
    gc = clean.backward(2.5).clone()
    for fill in ([NAN], [INF], [-INF] * c, [NAN, INF]):
        x = _t(cs.x)
        for i, v in enumerate(fill):
            x[ig, (c - 1 - i) % c] = v
        run = Run(x, y, cs.ignore)
        assert _same_bits(run.loss.reshape(1), clean.loss.reshape(1)) and _same_bits(run.backward(2.5), gc), fill


@pytest.mark.parametrize("c", [2, 9, 20, 129, 256])
def test_pred_of_a_nan_row_is_its_lowest_nan_column(c):
    from openscene_amd.losses import segmentation_loss
    cs = sb.case("gauss", sb.C_ROWS, c)
    x = _t(cs.x)
    lo, hi = c // 3, c - 1
    x[5, hi] = NAN
    x[5, lo] = NAN
    x[6, hi] = NAN
    x[6, 0] = INF
    x[7] = -INF
    _, pred = segmentation_loss(x, _t(cs.y), ignore_index=cs.ignore, pred=True)
    want = np.argmax(cs.x, axis=1)
    want[5], want[6], want[7] = lo, hi, 0
    assert np.array_equal(pred.cpu().numpy(), want)
    assert torch.equal(pred.cpu(), x.cpu().max(1)[1])


# ------------------------------------------------------------------------------------------------ the test-repeat vote
@pytest.mark.parametrize("c", [1, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256])
def test_votes_are_torchs_fp32_running_sum_bit_by_bit(c):
    """rows with duplicates and entries at -1 and n (they add nothing), three repeats; then a NaN logit reaches exactly the vote
    elements of the points that read its row, at its column."""
    from openscene_amd import ops
    n = 203
    n_pts = 3 * n + 7
    g = np.random.default_rng(sb._seed("vote", c))
    rows = g.integers(0, n, n_pts).astype(np.int64)
    rows[g.permutation(n_pts)[:20]] = np.repeat([-1, n], 10)
    rows_t = torch.from_numpy(rows)
    live = (rows_t >= 0) & (rows_t < n)
    store = torch.zeros(n_pts, c)
    votes = torch.zeros(n_pts, c, device=dev())
    for rep in range(3):
        xr = torch.from_numpy((4.0 * g.standard_normal((n, c))).astype(np.float32))
        store[live] = xr[rows_t[live]] + store[live]
        ops.seg_vote(xr.to(dev()), votes, rows=rows_t.to(dev()))
    assert _same_bits(votes.cpu(), store) and not votes[~live.to(dev())].any()
    xr = torch.from_numpy((4.0 * g.standard_normal((n, c))).astype(np.float32))
    bad_row, bad_col = int(rows_t[live][3]), c // 2
    xr[bad_row, bad_col] = NAN
    before = votes.clone()
    ops.seg_vote(xr.to(dev()), votes, rows=rows_t.to(dev()))
    want_nan = torch.zeros(n_pts, c, dtype=torch.bool)
    want_nan[torch.from_numpy(rows == bad_row), bad_col] = True
    assert want_nan.any() and torch.equal(torch.isnan(votes).cpu(), want_nan)
    store[live] = xr[rows_t[live]] + store[live]
    assert _same_bits(torch.nan_to_num(votes.cpu(), nan=0.0), torch.nan_to_num(store, nan=0.0))
    # without rows: votes[p] += logits[p]
    v2 = before[:n].clone()
    ops.seg_vote(xr.to(dev()), v2)
    assert _same_bits(torch.nan_to_num(v2.cpu(), nan=7.0), torch.nan_to_num(xr + before[:n].cpu(), nan=7.0))


# ------------------------------------------------------------------------------------------------ one optimizer step
@functools.lru_cache(maxsize=None)
def _opt_state(n):
    return tuple(torch.from_numpy(a).to(dev()) for a in sb.opt_state(n))


def _opt_ratio(got, ref, lim):
    """(worst err / limit, elements beyond it) on the device, in float64; a NaN is beyond every limit."""
    err = (got.double() - ref).abs()
    bad = int((~(err <= lim)).sum().item())
    ratio = torch.nan_to_num(torch.where(err == 0, torch.zeros_like(err), err / lim), nan=float("inf")).max().item()
    return ratio, bad


def _lib():
    from openscene_amd import ops
    return ops, ops._prep(dev())


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("kw", sb.SGD_SETTINGS, ids=lambda k: "m%g_d%g_n%d_wd%g" % (k["momentum"], k["dampening"], k["nesterov"], k["weight_decay"]))
def test_one_sgd_step_against_float64(kw, first):
    """osn_sgd_step from identical fp32 state against the update rule in float64 (on the device), every parameter and every
    momentum-buffer element within the limit of its own operand magnitudes (seg_bounds.sgd_step)."""
    from openscene_amd._lib import check
    ops, lib = _lib()
    lr = 0.05
    worst = 0.0
    for n in sb.OPT_SIZES:
        p0, g, b0, _ = _opt_state(n)
        rp, rb, lp, lbuf = sb.sgd_step(p0.double(), g.double(), b0.double(), lr, first=first, **kw)
        p, b = p0.clone(), b0.clone()
        with ops._Dev(dev()):
            check(lib.osn_sgd_step(ops._p(p), ops._p(g), ops._p(b if kw["momentum"] else None), n, lr, kw["momentum"], kw["dampening"],
                                   kw["weight_decay"], int(kw["nesterov"]), first, ops._stream(dev())), "osn_sgd_step")
        ratio, bad = _opt_ratio(p, rp, lp)
        assert not bad, "n = %d: %d parameters beyond the limit, worst %.3g" % (n, bad, ratio)
        worst = max(worst, ratio)
        if rb is not None:
            ratio, bad = _opt_ratio(b, rb, lbuf)
            assert not bad, "n = %d: %d buffer elements beyond the limit, worst %.3g" % (n, bad, ratio)
            worst = max(worst, ratio)
        else:
            assert _same_bits(b, b0)
    print("RATIO sgd %s first %d worst %.3f" % (kw, first, worst))


@pytest.mark.parametrize("kw", sb.ADAM_SETTINGS, ids=lambda k: "step%d_wd%g" % (k["step"], k["weight_decay"]))
def test_one_adam_step_against_float64(kw):
    from openscene_amd._lib import check
    ops, lib = _lib()
    hyper = (1e-3, 0.9, 0.999, 1e-8)
    worst = [0.0, 0.0, 0.0]
    for n in sb.OPT_SIZES:
        p0, g, m0, v0 = _opt_state(n)
        if kw["step"] == 1:
            m0, v0 = torch.zeros_like(m0), torch.zeros_like(v0)
        ref = sb.adam_step(p0.double(), g.double(), m0.double(), v0.double(), kw["step"], *hyper, kw["weight_decay"])
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        with ops._Dev(dev()):
            check(lib.osn_adam_step(ops._p(p), ops._p(g), ops._p(m), ops._p(v), n, kw["step"], *hyper, kw["weight_decay"],
                                    ops._stream(dev())), "osn_adam_step")
        for i, (name, got) in enumerate((("parameters", p), ("first moments", m), ("second moments", v))):
            ratio, bad = _opt_ratio(got, ref[i], ref[3 + i])
            assert not bad, "n = %d: %d %s beyond the limit, worst %.3g" % (n, bad, name, ratio)
            worst[i] = max(worst[i], ratio)
    print("RATIO adam %s worst p %.3f m %.3f v %.3f" % (kw, *worst))
