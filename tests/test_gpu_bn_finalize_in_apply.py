"""Batch-norm backward on the small maps (csrc/bn.hip): up to 64 row blocks of column sums (n <= 4096), with batch statistics, the apply
pass runs in groups of 32 columns, every workgroup adds the row blocks' partial sums of its columns itself (fold_sums: the finalize
kernel's tree) and the workgroups of the first 32 rows write ggamma and gbeta -- two launches instead of three.
osn_bn_set_separate_finalize(1) runs the three launches in the same process.

Every output (gx, gres, ggamma, gbeta) of the two-launch chain is compared BIT FOR BIT with the three-launch chain's, and held to the
per-column / per-element limits of tests/bn_bounds.py against its float64 reference.
  rows      1, 15, 16, 17, 63, 64, 65, 1023, 4095, 4096 (1, 1, 1, 1, 1, 1, 2, 16, 64, 64 row blocks: one partial, one group of eight
            not full, exactly two groups, all eight groups; 1 .. 128 row chunks of the apply pass, the last one ragged) and 4097
            (65 row blocks: stays on the finalize launch)
  columns   4, 60, 64, 68, 128, 256, 260: less than one 32-column group of the apply pass, a second group that is not full, exactly
            two, two and one quad, the widths of the deep U-Net levels, and eight groups and one quad (no width is too wide to fold)
  sources   1 to 3; source 0 and source 1 are column windows of wider matrices (ld > c)
  mask      none, from x (y null, beta given), from y
  gres      none, or stored by the column sums and read back by the apply pass
  earlier   osn_bn_set_flat_kernels(1) -- the flat apply kernels and one-row column sums, which always keep the three launches --
            gives the bits of the two-launch chain as well
  mode      batch statistics; evaluation mode (never folded: the apply pass needs no sums) gives the same bits under the switch too
  values    a NaN in source 0: it is in its column's gbeta, ggamma and gx, and in no other column, on both chains
The float64 reference is the slow part, so each shape checks the limits on one (configuration, source count) pair that rotates with
the shape; the bitwise comparison runs on every combination.

Measured on an MI355X, worst err / limit over all shapes: gx 0.28, gres 0.66 (three sources), ggamma 0.25, gbeta 0.49; every bitwise
comparison holds.  The module takes 5 s.
"""
import numpy as np
import pytest
import torch

import bn_bounds as bb

pytestmark = pytest.mark.gpu

NS = (1, 15, 16, 17, 63, 64, 65, 1023, 4095, 4096, 4097)
CS = (4, 60, 64, 68, 128, 256, 260)
SHAPES = [(n, c) for n in NS for c in CS]
NAMES = ("gx", "gres", "ggamma", "gbeta")
# (label, relu, y: none / with the residual, mask from x, gres)
CONFIGS = (("no mask", False, False, False, False), ("no mask, gres", False, False, False, True), ("mask from x", True, False, True, False),
           ("mask from y", True, True, False, False), ("mask from y, gres", True, True, False, True))
BOUNDED = (1, 4)                                             # the configurations held to the float64 reference: both store gres


def dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b, label):
    for name, u, v in zip(NAMES, a, b):
        assert (u is None) == (v is None), "%s: %s" % (label, name)
        if u is not None:
            assert torch.equal(_bits(u), _bits(v)), "%s: %s differs from the three-launch chain's" % (label, name)


def _both(ops, fn, label):
    """fn() with the finalize step inside the apply pass and as a launch of its own: the same bits.  -> the former's outputs"""
    new = fn()
    assert ops.bn_set_separate_finalize(True) is False
    try:
        old = fn()
    finally:
        assert ops.bn_set_separate_finalize(False) is True
    _same(new, old, label)
    return new


def _inputs(n, c):
    """Clean inputs (numpy, float32): columns at a common scale, sources of different magnitudes, and a residual moved so that no
    pre-activation of the training-mode forward pass lies within 3e-3 of zero (the float64 reference and the kernels then agree on
    every mask element)."""
    g = np.random.default_rng(bb._seed("finalize in apply", n, c))
    f = np.float32
    d = dict(x=(g.standard_normal((n, c)) * 2.5 + 0.7).astype(f), gamma=g.uniform(0.5, 1.5, c).astype(f),
             beta=(g.uniform(0.1, 0.5, c) * g.choice([-1.0, 1.0], c)).astype(f), res=g.standard_normal((n, c)).astype(f),
             wide0=g.standard_normal((n, c + 24)).astype(f), wide1=(3.0 * g.standard_normal((n, c + 8))).astype(f),
             g2=(0.25 * g.standard_normal((n, c))).astype(f))
    x8 = d["x"].astype(np.float64)
    pre = d["gamma"] * (x8 - x8.mean(0)) / np.sqrt(x8.var(0) + bb.EPS) + d["beta"] + d["res"]
    near = np.abs(pre) < 1e-3
    d["res"][near] += np.where(pre[near] >= 0, 4e-3, -4e-3).astype(f)
    return d


@pytest.mark.parametrize("n,c", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_finalize_in_the_apply_pass_gives_the_bits_of_the_finalize_launch(n, c):
    from openscene_amd import ops
    I = _inputs(n, c)
    x, gamma, beta, res = (_t(I[k]) for k in ("x", "gamma", "beta", "res"))
    wide0, wide1 = _t(I["wide0"]), _t(I["wide1"])
    gys = [wide0[:, 8:8 + c], wide1[:, 4:4 + c], _t(I["g2"])]
    gys_np = [I["wide0"][:, 8:8 + c], I["wide1"][:, 4:4 + c], I["g2"]]
    assert n == 1 or (gys[0].stride(0) > c and gys[1].stride(0) > c)
    rm, rv = torch.zeros(c, device=dev()), torch.ones(c, device=dev())
    y_res, mean, var = ops.bn_forward_train(x, gamma, beta, bb.EPS, res, True, rm.clone(), rv.clone(), bb.MOMENTUM)
    shape_index = SHAPES.index((n, c))
    bounded = (BOUNDED[shape_index % 2], 1 + (shape_index // 2) % 3)
    worst = {}

    def call(cfg, srcs, training=True):
        _, relu, with_y, from_x, want_gres = cfg
        return ops.bn_backward_multi(x, y_res if with_y else None, srcs, mean, var, gamma, bb.EPS, relu, training, want_gres,
                                     beta=beta if from_x else None)

    for k, cfg in enumerate(CONFIGS):
        for nsrc in (1, 2, 3):
            label = "%dx%d, %s, %d sources" % (n, c, cfg[0], nsrc)
            out = _both(ops, lambda: call(cfg, gys[:nsrc]), label)
            # the kernels of the earlier rounds (flat apply walk, one-row column sums; always three launches): the same bits
            assert ops.bn_set_flat_kernels(True) is False
            try:
                _same(out, call(cfg, gys[:nsrc]), label + ": the earlier rounds' kernels against the two-launch chain")
            finally:
                assert ops.bn_set_flat_kernels(False) is True
            if (k, nsrc) == bounded:
                r = bb.reference(x=I["x"], gamma=I["gamma"], beta=I["beta"], eps=bb.EPS, residual=I["res"] if cfg[2] else None, relu=cfg[1],
                                 gys=gys_np[:nsrc], training=True, momentum=bb.MOMENTUM, rm=np.zeros(c, np.float32), rv=np.ones(c, np.float32))
                L = bb.limits(r)
                assert L.excluded.mean() <= bb.EXCLUDED_CAP, "%s: %d of %d columns excluded" % (label, L.excluded.sum(), c)
                got = dict(zip(NAMES, (t.cpu().numpy() for t in out)))
                flat = bb.within(got, r, L, label, worst)
                print("RATIO %s %s" % (label, "  ".join("%s %.3f" % kv for kv in sorted(flat.items()))))
        # evaluation mode: the switch changes nothing there
        _both(ops, lambda: call(cfg, gys[:2], training=False), "%dx%d, %s, evaluation mode" % (n, c, cfg[0]))
    assert worst, "no configuration was held to the float64 reference"

    # a NaN in source 0 (row 0, column 1 % c), no mask: it reaches its column's two sums and, through them, every row of that column of gx
    poisoned = gys[0].clone()
    nan_col = 1 % c
    poisoned[0, nan_col] = float("nan")
    for nsrc in (1, 3):
        for cfg in (CONFIGS[0], CONFIGS[1]):
            label = "%dx%d, %s, %d sources, a NaN in source 0" % (n, c, cfg[0], nsrc)
            gx, gres, ggamma, gbeta = _both(ops, lambda: call(cfg, [poisoned] + gys[1:nsrc]), label)
            others = torch.ones(c, dtype=torch.bool, device=dev())
            others[nan_col] = False
            for name, t in (("gbeta", gbeta), ("ggamma", ggamma)):
                assert bool(torch.isnan(t[nan_col]).item()) and not bool(torch.isnan(t[others]).any().item()), "%s: %s" % (label, name)
            assert bool(torch.isnan(gx[:, nan_col]).all().item()) and not bool(torch.isnan(gx[:, others]).any().item()), "%s: gx" % label
            if gres is not None:
                assert int(torch.isnan(gres).sum().item()) == 1 and bool(torch.isnan(gres[0, nan_col]).item()), "%s: gres" % label


def test_the_switch_returns_the_previous_setting():
    from openscene_amd import ops
    assert ops.bn_set_separate_finalize(True) is False
    assert ops.bn_set_separate_finalize(True) is True
    assert ops.bn_set_separate_finalize(False) is True
    assert ops.bn_set_separate_finalize(False) is False
