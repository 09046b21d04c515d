"""What gives tests/test_gpu_seg_bounds.py its teeth, checked without a GPU: on every shape and input kind the GPU module uses, the
numpy emulation of the supervised head's arithmetic (seg_bounds.emulate) meets every limit of seg_bounds with a worst ratio <= 0.5,
the margin the limits have over correct arithmetic; the same emulation with ONE defect (seg_bounds.MUTANTS) breaks a limit on a named
case; the reference agrees with torch's float64 cross_entropy to 1e-12; the group, grid and q_s helpers are what csrc/seg.hip
computes; and one SGD / Adam step in emulated fp32 meets the per-element limits of seg_bounds.sgd_step / adam_step.

What the criteria of test_gpu_seg.py::test_loss_and_gradient_against_torch_float64 (the mean loss within 2e-6, the gradient matrix
within 1e-6 in relative L2) make of each mutant on that test's kind of inputs (scale * randn at scale 1 and 80, six of its shapes,
upstream gradient 1), and where the limits here see it (measured, asserted below; TABLE is printed by
test_each_mutant_breaks_a_limit):
    a  p = inv - 1.f where the label is the argmax    PASSES them; 3.2e5 x the gradient limit on confident rows (c = 2, 20, 160), also
                                                      beyond it on Gaussian rows at 37 x 16, 4097 x 129, 32769 x 20
    b  logf(1.f + s1) for log1pf(s1)                  PASSES them; 3.5e5 x the row-loss limit on confident rows; the MEAN loss limit
                                                      does not see it (a confident row's loss is lost in the mean): only the rows do
    c  upstream gradient ignored                      PASSES them (they never use one); 1.7e6 x the gradient limit at up = 2.5, -0.75
                                                      on every case
    d  butterfly started one step low                 caught there; here on every case with c >= 9 (gradient, loss and rows)
    e  8th value of a lane dropped                    caught there; here at c = 8, 16, 64, 256 (c > 7 G)
    f  loss partials without the later trips          caught there (100999 x 20); here at 4097 x 129 and 32769 x 20 (loss, 286 x)
    g  sc = up / n                                    caught there; here on every case (15 % of the labels are ignored)
    h  ignored rows left at sc softmax                caught there; here on every case (those rows are not bitwise +0)
    i  mean over the first 256 partials only          caught there; here at 2056 x 129, 4097 x 129, 32769 x 20 (loss and gradient)

Worst err / limit of the correct emulation over all cases and upstream gradients: gradient 0.446 (wide), mean loss 0.220 (gauss),
row loss 0.495 (confident).  The row loss of a two-class confident row is log1p of ONE term exp(-d): the counted roundings are
E_LOG1P + E_EXP + d + 1 = 5 + d, the correctly rounded emulation commits 2 + d of them at worst, so its ratio tends to 0.5 from below
as d grows to 100; it cannot pass it.
"""
import functools

import numpy as np
import pytest
import torch

import seg_bounds as sb

MARGIN = 0.5
C_CASES = [(k, n, c) for k in sb.KINDS for (n, c) in sb.C_SHAPES]
N_CASES = [(k, n, c) for k in sb.N_KINDS for (n, c) in sb.N_SHAPES]
# where each mutant is looked for: (kind, n, c)
MUTANT_CASES = [("confident", 37, 2), ("confident", 37, 20), ("confident", 37, 160), ("gauss", 37, 8), ("gauss", 37, 16),
                ("gauss", 37, 17), ("gauss", 37, 64), ("gauss", 37, 129), ("gauss", 37, 256), ("gauss", 257 * 8, 129),
                ("gauss", 512 * 8 + 1, 129), ("gauss", 512 * 64 + 1, 20)]
PASS_THE_OLD_CHECK = ("a", "b", "c")
WORST = {}


def _all_ups(cs, mutant=None):
    for up in sb.UPS:
        r = sb.reference(cs.x, cs.y, cs.ignore, up)
        yield up, r, sb.limits(r), sb.emulate(cs.x, cs.y, cs.ignore, up, mutant=mutant)


def _row_ratio(got, r, L):
    err = np.abs(got["val"][r.valid].astype(np.float64) - r.val[r.valid])
    return sb._worst(err, L.val[r.valid])


@pytest.mark.parametrize("kind,n,c", C_CASES + N_CASES, ids=["%s-%dx%d" % k for k in C_CASES + N_CASES])
def test_the_emulation_meets_every_limit_with_margin(kind, n, c):
    cs = sb.case(kind, n, c)
    for up, r, L, got in _all_ups(cs):
        label = "%s %d x %d up %g" % (kind, n, c, up)
        flat = sb.within(got, r, L, label)
        flat["val"], bad = _row_ratio(got, r, L)
        assert not bad, "%s: %d row losses beyond the limit (%.3g)" % (label, bad, flat["val"])
        print("RATIO %s %s" % (label, "  ".join("%s %.3f" % kv for kv in sorted(flat.items()))))
        for name, ratio in flat.items():
            assert ratio <= MARGIN, "%s: %s at %.3f of its limit: the derivation misses a term" % (label, name, ratio)
            WORST[(kind, name)] = max(WORST.get((kind, name), 0.0), ratio)
    print("WORST so far %s" % "  ".join("%s/%s %.3f" % (k[0], k[1], v) for k, v in sorted(WORST.items())))


def test_the_reference_agrees_with_torch_float64():
    for kind, n, c in [("gauss", 37, 20), ("confident", 37, 160), ("ties", 37, 9), ("big", 37, 256), ("gauss", 64, 8), ("wide", 37, 33)]:
        cs = sb.case(kind, n, c)
        for up in (1.0, -0.75):
            r = sb.reference(cs.x, cs.y, cs.ignore, up)
            xd = torch.from_numpy(np.array(cs.x)).double().requires_grad_()
            loss = torch.nn.functional.cross_entropy(xd, torch.from_numpy(np.array(cs.y)), ignore_index=cs.ignore)
            (loss * up).backward()
            assert abs(r.loss - loss.item()) <= 1e-12 * abs(loss.item())
            g = xd.grad.numpy()
            # (torch subtracts 1 from a rounded softmax: on a confident row its own error is 1e-16 absolute, not relative)
            assert (np.abs(r.grad - g) <= 1e-12 * np.abs(g) + 1e-15 * abs(r.s)).all()
            assert np.array_equal(r.pred, torch.from_numpy(np.array(cs.x)).max(1)[1].numpy())
            assert not r.grad[~r.valid].any()


def test_helpers_are_the_kernels_own():
    """seg_group / seg_grid (csrc/seg.hip:213-220), q_s, and the shapes: every bucket edge, the histogram switch, the grid-stride edge."""
    assert [sb.seg_group(c) for c in (1, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32]
    for c in range(1, 257):
        G = sb.seg_group(c)
        assert c <= sb.SEG_PER * G and (G == 1 or c > sb.SEG_PER * G // 2)
        assert sb.q_s(c) == (-(-c // G) - 1) + {1: 0, 2: 1, 4: 2, 8: 3, 16: 4, 32: 5}[G]
    assert (sb.q_s(1), sb.q_s(8), sb.q_s(9), sb.q_s(20), sb.q_s(160), sb.q_s(256)) == (0, 7, 5, 6, 9, 12)
    assert sb.seg_grid(1, 20) == 1 and sb.seg_grid(64, 20) == 1 and sb.seg_grid(65, 20) == 2
    assert sb.seg_grid(512 * 64, 20) == 512 and sb.seg_grid(512 * 64 + 1, 20) == 512 and sb.seg_grid(4097, 129) == 512
    assert sb.seg_grid(4096, 129) == 512 and sb.seg_grid(4088, 129) == 511
    assert {c for _, c in sb.C_SHAPES} >= {1, 2, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256}
    for c in sb.N_CLASSES:
        rpi = 256 // sb.seg_group(c)
        ns = [n for n, cc in sb.N_SHAPES if cc == c]
        assert ns == [1, rpi - 1, rpi, rpi + 1, 255 * rpi, 256 * rpi, 257 * rpi, 512 * rpi - 1, 512 * rpi + 1, 1024 * rpi + 3]
    assert max(n * c for n, c in sb.N_SHAPES) * 4 <= 8 * 2 ** 20 + 4096


def test_input_kinds_are_what_their_names_say():
    r = sb.reference(*sb.case("confident", 37, 20)[3:6])
    assert r.s1.min() < 1e-38 and r.s1.max() > 1e-4 and 0.5 < r.on_arg[r.valid].mean() < 1.0
    assert np.abs(r.p[np.arange(37), r.pred][r.on_arg]).min() < 1e-30
    cs = sb.case("big", 37, 20)
    assert np.abs(cs.x).min() > 9e3 and (cs.x > 0).any() and (cs.x < 0).any()
    cs = sb.case("ties", 37, 20)
    tied = (cs.x == cs.x.max(axis=1, keepdims=True)).sum(axis=1)
    assert (tied > 1).mean() > 0.5 and np.array_equal(cs.x, np.round(cs.x))
    r = sb.reference(*sb.case("wide", 37, 160)[3:6])
    assert r.dist.max() > 100 and ((r.dist > 87.4) & (r.dist < 104)).any()
    for k in sb.KINDS:
        for n, c in sb.C_SHAPES:
            cs = sb.case(k, n, c)
            assert cs.ignore == (255 if c < 256 else -100) and not cs.x.flags.writeable
            assert c == 1 or ((cs.y == cs.ignore).any() and (cs.y != cs.ignore).sum() >= 4)


@functools.lru_cache(maxsize=None)
def _old_ref(n, c, scale):
    x, y, ign = sb.old_inputs(n, c, scale)
    return x, y, ign, sb.reference(x, y, ign, 1.0)


def _old_verdict(mutant):
    """Do the older criteria pass the (mutated) emulation on every one of their shapes and scales?"""
    ok = True
    for n, c in sb.OLD_SHAPES:
        for scale in sb.OLD_SCALES:
            x, y, ign, r = _old_ref(n, c, scale)
            if r.n_valid:
                ok = ok and sb.old_check(sb.emulate(x, y, ign, 1.0, mutant=mutant), r)
    return ok


def test_the_correct_emulation_passes_the_older_criteria():
    assert _old_verdict(None)


@pytest.mark.parametrize("mutant", sb.MUTANTS)
def test_each_mutant_breaks_a_limit(mutant):
    broke = []
    for key in MUTANT_CASES:
        cs = sb.case(*key)
        for up, r, L, got in _all_ups(cs, mutant):
            res = sb.ratios(got, r, L)
            res["val"] = _row_ratio(got, r, L)
            bad = sorted(k for k, v in res.items() if v[1])
            if bad:
                broke.append((key, up))
                print("TABLE mutant %s %s up %g: beyond the limit: %s" % (mutant, key, up, {k: "%.3g" % res[k][0] for k in bad}))
    passed = _old_verdict(mutant)
    print("TABLE mutant %s: the criteria of test_loss_and_gradient_against_torch_float64 %s it" % (mutant, "PASS" if passed else "catch"))
    assert broke, "mutant %s stays inside every limit on every case" % mutant
    assert passed == (mutant in PASS_THE_OLD_CHECK), "mutant %s: the older criteria %s it" % (mutant, "pass" if passed else "catch")


def test_the_infinite_row_fix_leaves_finite_rows_alone():
    """csrc/seg.hip sets s1 to NaN when the row maximum is not finite; nothing else changed.  For a finite maximum the emulated
    arithmetic does not contain the new branch at all, and the GPU module compares two finite cases bit by bit with outputs recorded
    from the build before the fix (tests/golden/seg_parent_bits.npz)."""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seg_parent_bits.npz")
    z = np.load(path)
    for kind, n, c in sb.PARENT_CASES:
        key = "%s_%d_%d" % (kind, n, c)
        assert z[key + "_grad"].shape == (n, c) and z[key + "_grad"].dtype == np.int32 and z[key + "_loss"].dtype == np.int32
        # the recorded outputs are themselves within the limits (they are what the fixed kernel must reproduce bit by bit)
        cs = sb.case(kind, n, c)
        r = sb.reference(cs.x, cs.y, cs.ignore, 2.5)
        sb.within({"loss": z[key + "_loss"].view(np.float32)[0], "grad": z[key + "_grad"].view(np.float32)}, r, sb.limits(r), key)


# ------------------------------------------------------------------------------------------------ one optimizer step
def _f(a):
    return np.asarray(a, dtype=np.float64)


def _emulate_sgd(p, g, buf, lr, momentum, dampening, weight_decay, nesterov, first):
    """optim.hip:77-85 in fp32, every product and sum rounded (no fma)."""
    F = np.float32
    lr, mom, wd, omd = F(lr), F(momentum), F(weight_decay), F(1.0 - float(dampening))
    d = g.copy()
    if wd != 0:
        d = d + wd * p
    nbuf = None
    if mom != 0:
        nbuf = d if first else mom * buf + omd * d
        d = d + mom * nbuf if nesterov else nbuf
    out = p - lr * d
    assert out.dtype == F
    return out, nbuf


def _emulate_adam(p, g, m, v, step, lr, b1, b2, eps, wd):
    F = np.float32
    lr, b1, b2, eps, wd = F(lr), F(b1), F(b2), F(eps), F(wd)
    bc1 = F(1.0 - float(b1) ** step)
    bc2s = F(np.sqrt(1.0 - float(b2) ** step))
    ss = lr / bc1
    d = g.copy()
    if wd != 0:
        d = d + wd * p
    nm = m + (F(1) - b1) * (d - m)
    nv = b2 * v + (F(1) - b2) * d * d
    den = np.sqrt(nv) / bc2s + eps
    out = p - ss * nm / den
    assert out.dtype == F and nv.dtype == F
    return out, nm, nv


def _opt_ratio(got, ref, lim):
    return sb._worst(np.abs(_f(got) - ref), lim)


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("kw", sb.SGD_SETTINGS, ids=lambda k: "m%g_d%g_n%d_wd%g" % (k["momentum"], k["dampening"], k["nesterov"], k["weight_decay"]))
def test_an_emulated_sgd_step_meets_the_limits(kw, first):
    p, g, buf, _ = sb.opt_state(1028)
    rp, rb, lp, lbuf = sb.sgd_step(_f(p), _f(g), _f(buf), 0.05, first=first, **kw)
    gp, gb = _emulate_sgd(p, g, buf, 0.05, first=first, **kw)
    ratio, bad = _opt_ratio(gp, rp, lp)
    assert not bad and ratio <= MARGIN, ratio
    if rb is not None:
        ratio, bad = _opt_ratio(gb, rb, lbuf)
        assert not bad and ratio <= MARGIN, ratio
    # a defect the limit must see: the weight decay applied to the gradient twice, or a step with lr (1 + 3e-6)
    if kw["weight_decay"]:
        wrong, _ = _emulate_sgd(p, g + np.float32(kw["weight_decay"]) * p, buf, 0.05, first=first, **kw)
        assert _opt_ratio(wrong, rp, lp)[1] > 0
    wrong, _ = _emulate_sgd(p, g, buf, 0.05 * (1 + 3e-6), first=first, **kw)
    assert _opt_ratio(wrong, rp, lp)[1] > 0


@pytest.mark.parametrize("kw", sb.ADAM_SETTINGS, ids=lambda k: "step%d_wd%g" % (k["step"], k["weight_decay"]))
def test_an_emulated_adam_step_meets_the_limits(kw):
    p, g, m, v = sb.opt_state(1028)
    if kw["step"] == 1:
        m, v = np.zeros_like(m), np.zeros_like(v)
    ref = sb.adam_step(_f(p), _f(g), _f(m), _f(v), kw["step"], 1e-3, 0.9, 0.999, 1e-8, kw["weight_decay"])
    got = _emulate_adam(p, g, m, v, kw["step"], 1e-3, 0.9, 0.999, 1e-8, kw["weight_decay"])
    for i in range(3):
        ratio, bad = _opt_ratio(got[i], ref[i], ref[3 + i])
        assert not bad and ratio <= MARGIN, (i, ratio)
    # a defect the limit must see: the second moment's bias correction left out of the denominator
    if kw["step"] == 1:
        bc2s = np.float32(np.sqrt(1.0 - float(np.float32(0.999))))
        wrong = p - (np.float32(1e-3) / np.float32(1.0 - float(np.float32(0.9)))) * got[1] / (np.sqrt(got[2]) + np.float32(1e-8))
        assert bc2s < 0.1 and _opt_ratio(wrong, ref[0], ref[3])[1] > 0
