"""Batch-norm backward with a residual destination (csrc/bn.hip): the column-sum pass stores gres = the masked sum of the gradient
sources and the apply pass reads it back (col_reduce_gres_kernel, bn_bwd_apply_gres_kernel), instead of both passes forming it.

Shapes: n in {1, 15, 16, 17, 63, 64, 65, 200, 33000} x c in {4, 60, 64, 68, 96} -- 16 = the reduction's row lanes (CR_RL), 64 = four
times that and its column group (CR_COLS), 33000 > 512 x 64 rows makes rows_per_block > 64, 96 half-fills the second column group.
Every shape runs 1, 2 and 3 sources (source 0 a column window of a wider matrix), ReLU on and off, training and evaluation mode:

  * gres bitwise equal to where(y > 0, (g0 + g1) + g2, 0) evaluated in fp32 by torch on the device (IEEE adds in that association:
    equality is exact), on inputs whose y holds NaN, +0 and -0 and whose sources hold NaN under open and closed mask elements,
    and on the clean inputs of the sums check;
  * gx, ggamma, gbeta (and gres) within the per-column / per-element limits of tests/bn_bounds.py against its float64 reference.
    The float64 reference is the slow part (long-double column sums): below 33000 rows every (ReLU, mode) pair is checked with a
    source count that rotates with the shape; at 33000 rows, where n only changes rows_per_block (a loop bound that no mode flag
    touches), each shape checks two of the four pairs, rotating with c, so that every pair is checked at that size as well;
  * two calls on the same inputs agree bitwise in every output;
  * the aliasing rule of include/openscene_amd.h: gres written in place over source 0 takes the two-pass data flow and gives
    bitwise the results of the call with a separate gres.

Measured on an MI355X, worst err / limit over all shapes: gx 0.27, gres 0.66 (against the float64 sum; three sources), ggamma 0.30,
gbeta 0.50; the bitwise checks hold on every case.  The module takes 5 s.
"""
import numpy as np
import pytest
import torch

import bn_bounds as bb

pytestmark = pytest.mark.gpu

NS = (1, 15, 16, 17, 63, 64, 65, 200, 33000)
CS = (4, 60, 64, 68, 96)
SHAPES = [(n, c) for n in NS for c in CS]
MODES = [(True, True), (True, False), (False, True), (False, False)]          # (relu, training)
BIG = 33000


def dev():
    return torch.device("cuda", 0)


def _ops():
    from openscene_amd import ops
    return ops


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b, label):
    for name, u, v in zip(("gx", "gres", "ggamma", "gbeta"), a, b):
        assert torch.equal(_bits(u), _bits(v)), "%s: %s differs" % (label, name)


def _expected_gres(y, gys, relu):
    g = gys[0]
    for s in gys[1:]:
        g = g + s                                            # (g0 + g1) + g2 in fp32
    return torch.where(y > 0, g, torch.zeros_like(g)) if relu else g.clone()


def _inputs(n, c):
    """Clean inputs of one shape (numpy, float32): columns at a common scale, gradient sources of different magnitudes."""
    g = np.random.default_rng(bb._seed("gres", n, c))
    f = np.float32
    d = dict(x=(g.standard_normal((n, c)) * 2.5 + 0.7).astype(f), gamma=g.uniform(0.5, 1.5, c).astype(f),
             beta=(g.uniform(0.1, 0.5, c) * g.choice([-1.0, 1.0], c)).astype(f), res=g.standard_normal((n, c)).astype(f),
             wide=g.standard_normal((n, c + 24)).astype(f), g1=(3.0 * g.standard_normal((n, c))).astype(f),
             g2=(0.25 * g.standard_normal((n, c))).astype(f))
    d["rm"] = (d["x"].mean(0) * (1 + 0.1 * g.standard_normal(c))).astype(f)
    d["rv"] = ((d["x"].var(0) + 0.5) * g.uniform(0.5, 2.0, c)).astype(f)
    # One residual per mode, moved so that no pre-activation lies within 3e-3 of zero: three decades above the y limit at these
    # magnitudes, so the float64 reference and the kernels agree on every ReLU mask element and no column has to be left out.
    x8 = d["x"].astype(np.float64)
    for name, m, v in (("res", x8.mean(0), x8.var(0)), ("res_eval", d["rm"].astype(np.float64), d["rv"].astype(np.float64))):
        r = d["res"].copy()
        pre = d["gamma"] * (x8 - m) / np.sqrt(v + bb.EPS) + d["beta"] + r
        near = np.abs(pre) < 1e-3
        r[near] += np.where(pre[near] >= 0, 4e-3, -4e-3).astype(f)
        d[name] = r
    return d


def _modes_checked_against_float64(n, c):
    if n < BIG:
        return MODES
    k = CS.index(c)
    return [MODES[k % 4], MODES[(k + 2) % 4]]


@pytest.mark.parametrize("n,c", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_gres_is_exact_and_the_sums_stay_within_their_limits(n, c):
    ops = _ops()
    I = _inputs(n, c)
    x, gamma, beta, res, res_eval, rm, rv = (_t(I[k]) for k in ("x", "gamma", "beta", "res", "res_eval", "rm", "rv"))
    wide = _t(I["wide"])
    gys = [wide[:, 8:8 + c], _t(I["g1"]), _t(I["g2"])]
    gys_np = [I["wide"][:, 8:8 + c], I["g1"], I["g2"]]
    shape_index = SHAPES.index((n, c))
    worst = {}
    # ---- a y with NaN, +0 and -0, and sources with NaN under open and closed mask elements: gres exact, calls repeatable
    rng = np.random.default_rng(bb._seed("gres y", n, c))
    y_np = rng.standard_normal((n, c)).astype(np.float32)
    special = np.array([np.nan, 0.0, -0.0], dtype=np.float32)
    for r in sorted({0, n // 2, n - 1}):
        cols = rng.permutation(c)[:3]
        y_np[r, cols] = special[:len(cols)]
    y_odd = _t(y_np)
    poisoned = [s.clone() for s in gys]
    for k, (r, j) in enumerate([(0, 0), (n - 1, c - 1), (n // 2, c // 2), (n // 3, 1), (n - 1, 0), (0, c - 1)]):
        poisoned[k % 3][r, j] = float("nan")
    mean, var = rm, rv + 0.5
    for relu, training in MODES:
        for nsrc in (1, 2, 3):
            label = "%dx%d odd y, relu %d training %d, %d sources" % (n, c, relu, training, nsrc)
            out = ops.bn_backward_multi(x, y_odd, poisoned[:nsrc], mean, var, gamma, bb.EPS, relu, training, True)
            want = _expected_gres(y_odd, poisoned[:nsrc], relu)
            assert torch.equal(_bits(out[1]), _bits(want)), "%s: gres is not the masked fp32 sum" % label
            _same(out, ops.bn_backward_multi(x, y_odd, poisoned[:nsrc], mean, var, gamma, bb.EPS, relu, training, True), label + ", second call")
    # ---- clean inputs, y from the forward pass: gres exact, sums and gx against the float64 reference
    for m, (relu, training) in enumerate(MODES):
        if training:
            y, mean, var = ops.bn_forward_train(x, gamma, beta, bb.EPS, res, relu, rm.clone(), rv.clone(), bb.MOMENTUM)
        else:
            y, mean, var = ops.bn_apply(x, rm, rv, gamma, beta, bb.EPS, res_eval, relu), rm, rv
        against64 = (relu, training) in _modes_checked_against_float64(n, c)
        ref = None
        for nsrc in (1, 2, 3):
            label = "%dx%d relu %d training %d, %d sources" % (n, c, relu, training, nsrc)
            out = ops.bn_backward_multi(x, y, gys[:nsrc], mean, var, gamma, bb.EPS, relu, training, True)
            assert torch.equal(_bits(out[1]), _bits(_expected_gres(y, gys[:nsrc], relu))), "%s: gres is not the masked fp32 sum" % label
            if against64 and nsrc == 1 + (shape_index + m) % 3:
                if ref is None:
                    a = dict(x=I["x"], gamma=I["gamma"], beta=I["beta"], eps=bb.EPS, residual=I["res" if training else "res_eval"], relu=relu, gys=None,
                             training=training)
                    a.update(dict(momentum=bb.MOMENTUM, rm=I["rm"], rv=I["rv"]) if training else dict(mean=I["rm"], var=I["rv"]))
                    ref = bb.reference(**a)
                r = bb.with_sources(ref, gys_np[:nsrc])
                L = bb.limits(r)
                assert L.excluded.mean() <= bb.EXCLUDED_CAP, "%s: %d of %d columns excluded" % (label, L.excluded.sum(), c)
                got = dict(zip(("gx", "gres", "ggamma", "gbeta"), (t.cpu().numpy() for t in out)))
                flat = bb.within(got, r, L, label, worst)
                print("RATIO %s %s" % (label, "  ".join("%s %.3f" % kv for kv in sorted(flat.items()))))
    print("WORST %dx%d %s" % (n, c, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("n,c", [(17, 4), (200, 96), (BIG, 68)])
def test_a_gres_that_overlaps_source_0_gives_the_bits_of_a_separate_gres(n, c):
    """gres written in place over source 0 (contiguous): the library keeps the data flow in which both passes form g and the apply
    pass writes gres element by element, each element after its own read.  Same bits as the call that gets a gres of its own."""
    ops = _ops()
    I = _inputs(n, c)
    x, gamma, beta, res, res_eval, rm, rv = (_t(I[k]) for k in ("x", "gamma", "beta", "res", "res_eval", "rm", "rv"))
    g0, g1 = _t(I["g2"]), _t(I["g1"])
    for relu, training in MODES:
        if training:
            y, mean, var = ops.bn_forward_train(x, gamma, beta, bb.EPS, res, relu, rm.clone(), rv.clone(), bb.MOMENTUM)
        else:
            y, mean, var = ops.bn_apply(x, rm, rv, gamma, beta, bb.EPS, res_eval, relu), rm, rv
        for srcs in ([g0], [g0, g1]):
            label = "%dx%d relu %d training %d, %d sources" % (n, c, relu, training, len(srcs))
            apart = ops.bn_backward_multi(x, y, srcs, mean, var, gamma, bb.EPS, relu, training, True)
            assert torch.equal(_bits(apart[1]), _bits(_expected_gres(y, srcs, relu))), label
            inplace = g0.clone()
            over = ops.bn_backward_multi(x, y, [inplace] + srcs[1:], mean, var, gamma, bb.EPS, relu, training, True, gres_out=inplace)
            assert over[1].data_ptr() == inplace.data_ptr()
            _same(apart, over, label + ", gres over source 0")
