"""The batch-norm kernels (csrc/bn.hip) against the per-column and per-element limits of tests/bn_bounds.py, at the edges of their own
code -- the row lanes and row blocks of the column reduction, the finalize iterations and the 512-block cap, the 8-column workgroups
and the 4096-row switch of the single-launch kernel -- on inputs whose columns differ by six decades ("scales") or sit at a mean / std
of up to 4096 ("offset").  Every test calls the ops.* wrappers directly.  test_bn_bounds_cpu.py shows that these limits separate
the kernels' arithmetic (ratio <= 0.5) from seven single defects, four of which the tensor-max checks of test_gpu_dense.py let pass.

Also: constant and nearly constant columns; bitwise repeatability; the single-launch kernel against the three-launch path at 4096
rows; and the isolation of columns under non-finite values -- a NaN or inf in x makes its own column NaN in training mode (through
the ReLU as well: torch.relu propagates NaN) and touches no bit of any other column.

Worst err / limit per quantity: NOT MEASURED on an MI355X yet -- no GPU could be reached while this module was written; every test
prints its figures ("RATIO ..." per launch, "WORST ..." per case) and they belong here once a run exists.  The numpy emulation of the
kernels' arithmetic (test_bn_bounds_cpu.py, shapes up to 8193 rows) gives, worst over all cases:
    y 0.50  mean 0.50  var 0.49  running_mean 0.34  running_var 0.36  gx 0.50  gres 0.66 (three sources)  ggamma 0.50  gbeta 0.48
"""
import numpy as np
import pytest
import torch

import bn_bounds as bb

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def _ops():
    from openscene_amd import ops
    return ops


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _n(t):
    return None if t is None else t.detach().cpu().numpy()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class OnDevice:
    """A case's inputs on the device; source 0 of the gradient is a column window of a wider matrix there as well."""

    def __init__(self, cs):
        self.cs = cs
        for name in ("x", "gamma", "beta", "res", "res_eval", "rm", "rv"):
            setattr(self, name, _t(getattr(cs, name)))
        self.wide = _t(cs.wide)
        self.gys = [self.wide[:, 8:8 + cs.c], _t(cs.gys[1]), _t(cs.gys[2])]

    def residual(self, config):
        return {"plain": None, "res": self.res, "mask": None, "eval": self.res_eval}[config]

    def forward(self, config, x=None, window=None):
        """Training-mode forward of a configuration -> {name: tensor}; window: a [n, c] column window that receives y as well."""
        ops = _ops()
        x = self.x if x is None else x
        rm, rv = self.rm.clone(), self.rv.clone()
        a = (x, self.gamma, self.beta, bb.EPS, self.residual(config), config != "plain", rm, rv, bb.MOMENTUM)
        y, mean, var = ops.bn_forward_train(*a, y2=window)
        return dict(y=y, mean=mean, var=var, rm=rm, rv=rv)


_BWD = ("gx", "gres", "ggamma", "gbeta")


def _bwd(out):
    return dict(zip(_BWD, out))


def _all_same_bits(a, b, label):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] is None and b[k] is None) or _same_bits(a[k], b[k]), "%s: %s differs" % (label, k)


def _check(got, r, L, label, worst):
    flat = bb.within({k: _n(v) for k, v in got.items()}, r, L, label, worst)
    print("RATIO %s %s" % (label, "  ".join("%s %.3f" % kv for kv in sorted(flat.items()))))


CASES = [(k, n, c) for (n, c) in bb.SHAPES for k in bb.GPU_KINDS]


@pytest.mark.parametrize("kind,n,c", CASES, ids=["%s-%dx%d" % k for k in CASES])
def test_per_column_and_per_element_limits(kind, n, c):
    ops = _ops()
    cs = bb.case(kind, n, c)
    D = OnDevice(cs)
    worst = {}
    tag = "%s %dx%d" % (kind, n, c)
    with_window = bb.SHAPES.index((n, c)) % 3 == 0
    for config in ("plain", "res", "mask"):
        label = "%s %s" % (tag, config)
        args = bb.config_args(cs, config, 3)
        r = bb.reference(**args)
        L = bb.limits(r)
        assert L.excluded.mean() <= bb.EXCLUDED_CAP, "%s: %d of %d columns excluded" % (label, L.excluded.sum(), c)
        fwd = D.forward(config)
        _check(fwd, r, L, label, worst)
        _all_same_bits(fwd, D.forward(config), label + ", second call")
        if with_window:                                      # the same launch with a second destination inside a wider matrix
            cat = torch.full((n, c + 40), -7.0, device=dev())
            _all_same_bits(fwd, D.forward(config, window=cat[:, 16:16 + c]), label + ", with a window")
            assert _same_bits(cat[:, 16:16 + c], fwd["y"]) and bool((cat[:, :16] == -7).all()) and bool((cat[:, 16 + c:] == -7).all())
        y, mean, var = fwd["y"], fwd["mean"], fwd["var"]
        if config == "plain":
            out = _bwd(ops.bn_backward(D.x, None, D.gys[1], mean, var, D.gamma, bb.EPS, False, True, False))
            r1 = bb.with_sources(r, [cs.gys[1]])
            _check(out, r1, bb.limits(r1), label + " backward", worst)
        elif config == "res":
            for nsrc in (1, 2, 3):                           # 1 .. 3 gradient sources, the first a column window
                rk = r if nsrc == 3 else bb.with_sources(r, list(cs.gys[:nsrc]))
                out = _bwd(ops.bn_backward_multi(D.x, y, D.gys[:nsrc], mean, var, D.gamma, bb.EPS, True, True, True))
                _check(out, rk, bb.limits(rk) if nsrc < 3 else L, "%s backward, %d sources" % (label, nsrc), worst)
            _all_same_bits(out, _bwd(ops.bn_backward_multi(D.x, y, D.gys, mean, var, D.gamma, bb.EPS, True, True, True)), label + " backward, second call")
        else:                                                # the mask read from y and the mask recomputed from x, three sources
            out = _bwd(ops.bn_backward_multi(D.x, y, D.gys, mean, var, D.gamma, bb.EPS, True, True, False))
            again = _bwd(ops.bn_backward_multi(D.x, None, D.gys, mean, var, D.gamma, bb.EPS, True, True, False, beta=D.beta))
            _all_same_bits(out, again, label + ": mask from y against mask from x")
            _check(out, r, L, label + " backward, 3 sources", worst)
    # evaluation mode (mean / var = the running buffers) with a residual and ReLU
    label = tag + " eval"
    args = bb.config_args(cs, "eval", 3)
    r = bb.reference(**args)
    L = bb.limits(r)
    assert L.excluded.mean() <= bb.EXCLUDED_CAP, "%s: %d of %d columns excluded" % (label, L.excluded.sum(), c)
    y = ops.bn_apply(D.x, D.rm, D.rv, D.gamma, D.beta, bb.EPS, D.res_eval, True)
    assert _same_bits(y, ops.bn_apply(D.x, D.rm, D.rv, D.gamma, D.beta, bb.EPS, D.res_eval, True))
    out = _bwd(ops.bn_backward_multi(D.x, y, D.gys, D.rm, D.rv, D.gamma, bb.EPS, True, False, True))
    _check(dict(out, y=y), r, L, label, worst)
    print("WORST %s %s" % (tag, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("n", [513, 4161])
def test_constant_and_nearly_constant_columns(n):
    """Column 0 constant (var = 0), column 1 = 4096 + 2^-10 randn (the fp64 s2 / n - m^2 keeps about 3 digits of the variance and may come
    out negative before the clamp), both on the single-launch and on the three-launch path: var >= 0 and finite, y within its limit
    (in the constant column that is beta + residual), gx finite and within its limit."""
    ops = _ops()
    c = 12
    g = np.random.default_rng(n)
    x = g.standard_normal((n, c)).astype(np.float32)
    x[:, 0] = 3.25
    x[:, 1] = (4096 + 2.0 ** -10 * g.standard_normal(n)).astype(np.float32)
    gamma = g.uniform(0.5, 1.5, c).astype(np.float32)
    beta = g.uniform(-0.5, 0.5, c).astype(np.float32)
    res = g.standard_normal((n, c)).astype(np.float32)
    gy = g.standard_normal((n, c)).astype(np.float32)
    rm, rv = np.zeros(c, np.float32), np.ones(c, np.float32)
    args = dict(x=x, gamma=gamma, beta=beta, eps=bb.EPS, residual=res, relu=False, gys=[gy], training=True, momentum=bb.MOMENTUM, rm=rm, rv=rv)
    r = bb.reference(**args)
    L = bb.limits(r)
    assert r.var[0] == 0 and r.var[1] < 2e-6 and not L.excluded.any()
    xd, gad, bed, rmd, rvd = _t(x), _t(gamma), _t(beta), _t(rm), _t(rv)
    y, mean, var = ops.bn_forward_train(xd, gad, bed, bb.EPS, _t(res), False, rmd, rvd, bb.MOMENTUM)
    assert bool(torch.isfinite(var).all()) and bool((var >= 0).all()) and bool(torch.isfinite(rvd).all()) and bool((rvd >= 0).all())
    out = _bwd(ops.bn_backward(xd, None, _t(gy), mean, var, gad, bb.EPS, False, True, True))
    assert bool(torch.isfinite(out["gx"]).all()) and bool(torch.isfinite(y).all())
    worst = {}
    _check(dict(out, y=y, mean=mean, var=var, rm=rmd, rv=rvd), r, L, "degenerate columns, %d rows" % n, worst)
    assert float((y[:, 0] - _t(beta)[0] - _t(res)[:, 0]).abs().max()) <= float(L.y[:, 0].max())
    # the three-launch statistics on the same x (512 rows run the single-launch kernel above, 4161 do not: both reductions see the columns)
    m2, v2 = ops.bn_stats(xd)
    assert bool(torch.isfinite(v2).all()) and bool((v2 >= 0).all())
    bb.within(dict(mean=_n(m2), var=_n(v2)), r, L, "degenerate columns, bn_stats, %d rows" % n, worst)


def test_single_launch_kernel_agrees_with_the_three_launch_path_at_4096_rows():
    """4096 rows: bn_forward_train runs the single-workgroup kernel, bn_stats + bn_apply the three launches.  Their statistics agree
    within the statistics limits; bn_apply fed the single-launch kernel's own mean / var gives y BITWISE (one bn_val on both paths)."""
    ops = _ops()
    for kind in bb.GPU_KINDS:
        cs = bb.case(kind, 4096, 68)
        D = OnDevice(cs)
        r = bb.reference(**bb.config_args(cs, "res", 0))
        L = bb.limits(r)
        one = D.forward("res")
        rm, rv = D.rm.clone(), D.rv.clone()
        m3, v3 = ops.bn_stats(D.x, rm, rv, bb.MOMENTUM)
        worst = {}
        _check(one, r, L, "%s single launch" % kind, worst)
        _check(dict(mean=m3, var=v3, rm=rm, rv=rv), r, L, "%s three launches" % kind, worst)
        assert bool(((one["mean"] - m3).abs().double().cpu() <= torch.from_numpy(2 * L.mean)).all())
        assert bool(((one["var"] - v3).abs().double().cpu() <= torch.from_numpy(2 * L.var)).all())
        y3 = ops.bn_apply(D.x, one["mean"], one["var"], D.gamma, D.beta, bb.EPS, D.res, True)
        assert _same_bits(y3, one["y"]), "%s: bn_apply on the single-launch kernel's statistics differs from its y" % kind


def _columns_but(t, j):
    keep = torch.ones(t.shape[-1], dtype=torch.bool, device=t.device)
    keep[j] = False
    return t[..., keep]


@pytest.mark.parametrize("n,c", [(513, 20), (4161, 36)])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_a_non_finite_x_stays_in_its_column(n, c, relu, poison):
    """Training mode: NaN (or +inf: mean = inf, var = inf - inf) at one x[r, j] makes mean, var, the running buffers and ALL of y[:, j] NaN, with
    and without the ReLU, and leaves every other column of every output bitwise what it was.  Evaluation mode: only y[r, j] is NaN."""
    ops = _ops()
    cs = bb.case("scales", n, c)
    D = OnDevice(cs)
    config = "res" if relu else "plain"
    r_, j = n - 2, 5
    clean = D.forward(config)
    assert all(bool(torch.isfinite(v).all()) for v in clean.values())
    x2 = D.x.clone()
    x2[r_, j] = poison
    got = D.forward(config, x=x2)
    for name in ("mean", "var", "rm", "rv"):                 # (the mean of a column that holds +inf is +inf, as in torch; its variance is inf - inf)
        want_inf = poison == poison and name in ("mean", "rm")
        ok = float(got[name][j]) == float("inf") if want_inf else bool(torch.isnan(got[name][j]))
        assert ok, "%s[%d] = %r" % (name, j, float(got[name][j]))
    assert bool(torch.isnan(got["y"][:, j]).all()), "%d of %d elements of y[:, j] are not NaN" % (int((~torch.isnan(got["y"][:, j])).sum()), n)
    for name in got:
        assert _same_bits(_columns_but(got[name], j), _columns_but(clean[name], j)), "%s changed outside column %d" % (name, j)
    if poison != poison:
        res = D.res_eval if relu else None
        y0 = ops.bn_apply(D.x, D.rm, D.rv, D.gamma, D.beta, bb.EPS, res, relu)
        y1 = ops.bn_apply(x2, D.rm, D.rv, D.gamma, D.beta, bb.EPS, res, relu)
        where = torch.isnan(y1)
        assert int(where.sum()) == 1 and bool(where[r_, j]), "evaluation mode: NaN at %s" % where.nonzero().tolist()[:4]
        y1[r_, j] = y0[r_, j]
        assert _same_bits(y0, y1)


@pytest.mark.parametrize("n,c", [(513, 20), (4161, 36)])
def test_a_nan_gradient_stays_in_its_column_and_under_a_closed_relu_is_dropped(n, c):
    ops = _ops()
    cs = bb.case("scales", n, c)
    D = OnDevice(cs)
    j = 5
    fwd = D.forward("res")
    y, mean, var = fwd["y"], fwd["mean"], fwd["var"]
    open_rows, closed_rows = (y[:, j] > 0).nonzero().reshape(-1), (y[:, j] <= 0).nonzero().reshape(-1)
    assert open_rows.numel() and closed_rows.numel()

    def backward(gys, y_, want_gres=True, beta=None):
        return _bwd(ops.bn_backward_multi(D.x, y_, gys, mean, var, D.gamma, bb.EPS, True, True, want_gres, beta=beta))

    clean = backward(D.gys, y)
    assert all(bool(torch.isfinite(v).all()) for v in clean.values())
    g1 = D.gys[1].clone()
    r_open = int(open_rows[-1])
    g1[r_open, j] = float("nan")
    got = backward([D.gys[0], g1, D.gys[2]], y)
    assert bool(torch.isnan(got["gx"][:, j]).all()) and bool(torch.isnan(got["ggamma"][j])) and bool(torch.isnan(got["gbeta"][j]))
    where = torch.isnan(got["gres"])
    assert int(where.sum()) == 1 and bool(where[r_open, j])
    for name in ("gx", "ggamma", "gbeta", "gres"):
        assert _same_bits(_columns_but(got[name], j), _columns_but(clean[name], j)), "%s changed outside column %d" % (name, j)
    g1 = D.gys[1].clone()
    g1[int(closed_rows[-1]), j] = float("nan")
    _all_same_bits(backward([D.gys[0], g1, D.gys[2]], y), clean, "a NaN gradient under a closed ReLU")
    # the same with the mask recomputed from x (ReLU without a residual)
    fwd = D.forward("mask")
    y, mean, var = fwd["y"], fwd["mean"], fwd["var"]
    closed_rows = (y[:, j] <= 0).nonzero().reshape(-1)
    assert closed_rows.numel()
    clean = backward(D.gys, None, False, D.beta)
    g1 = D.gys[1].clone()
    g1[int(closed_rows[0]), j] = float("nan")
    _all_same_bits(backward([D.gys[0], g1, D.gys[2]], None, False, D.beta), clean, "a NaN gradient under a closed ReLU, mask from x")
