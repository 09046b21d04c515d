"""The arithmetic contract of batch norm in one place (plain helper module; imported by test_bn_bounds_cpu.py and
test_gpu_bn_bounds.py): a float64 / long-double reference, per-element and per-column limits derived from the roundings of the
kernels' own expressions, a numpy emulation of that arithmetic, and the emulation with one defect at a time (MUTANTS).

Kernel arithmetic (csrc/bn.hip, csrc/epilogue.h): column sums of x and x^2 in fp64, m = s1 / n, v = max(s2 / n - m^2, 0) in fp64,
both rounded to fp32; is = 1 / sqrt(v + eps) in fp32; y = relu(fma((x - mu) * is, ga, be) + res) in fp32.  Backward: g = the fp32
sum of the sources under the mask y > 0, fp64 column sums of g and g * xhat rounded to fp32, and
gx = ga * is * (g - sum_g / n - xhat * sum_gx / n) in fp32 with inv_n = 1.f / float(n).

Limits, u = 2^-24 (one fp32 rounding), every constant twice what the first-order count of roundings gives:
    mean[j]     2u |m|
    var[j]      2u v + 8 * 2^-52 E[x^2]          (the second term: s2 / n - m^2 cancels in fp64)
    running_*   the limit above times momentum (times n / (n - 1) for the variance), plus the four fp32 roundings of
                (1 - momentum) * r + momentum * s:  u (4 |(1 - momentum) r| + 2 |momentum s| + 2 |result|)
    y[r, j]     u (16 |ga xhat| + 2 |ga is m| + 4 |be| + 4 |res| + 4 |pre|) + |ga xhat| dv[j]
                dv = 8 * 2^-52 E[x^2] / (v + eps): the relative error that the cancellation leaves in v + eps (0 in evaluation
                mode, where mean and var are inputs); pre: the value before the ReLU.  ReLU is 1-Lipschitz, so the same limit
                holds behind it; an element with |pre| <= its limit may be on either side ("unclear").
    gres        exact under a clear mask with one source; with k > 1 sources k u sum_i |g_i| (their fp32 sum)
    gbeta[j]    2u |sum g| + 2^-49 sum |g| + sum_r dg
    ggamma[j]   2u |sum g xhat| + 2 sum_r |g| dxhat + 2^-49 sum |g xhat| + sum_r dg |xhat|
                dxhat = u (3 |xhat| + |is m|) + |xhat| dv
    gx[r, j]    (16u + dv) |ga is| (|g| + |sum g| / n + |xhat sum g xhat| / n)
                + 2 |ga is| (dxhat |sum g xhat| / n + |xhat| sum_r(dxhat |g|) / n)
                + 2 |ga is| (dg + sum_r dg / n + |xhat| sum_r(dg |xhat|) / n)
    dg = (k - 1) u sum_i |g_i| is the rounding of the k-source sum (0 for one source); the dv in the first gx term is the relative
    error of the factor ga * is, which the cancellation in v reaches as it reaches xhat.  Every limit has the absolute floor 1e-37.
A column in which any element is unclear is left out of the BACKWARD checks (a flipped mask element changes the whole column's
sums); at most EXCLUDED_CAP of a case's columns may be, and cases() moves pre-activations away from zero so that the reference
alone meets that.
"""
import collections
import copy
import functools
import types
import zlib

import numpy as np

U = 2.0 ** -24
C64 = 8 * 2.0 ** -52
FLOOR = 1e-37
EPS = 1e-5
MOMENTUM = 0.1
EXCLUDED_CAP = 0.05
KINDS = ("scales", "offset", "plain")
GPU_KINDS = ("scales", "offset")
MUTANTS = ("a", "b", "c", "d", "e", "f", "g")
# (n, c): the edges of col_reduce (16 row lanes, 64-row blocks, 64 columns), of the finalize kernel (16 columns, 64 slices per
# iteration, the 512-block cap at 32768 rows) and of the single-workgroup kernel (8 columns, 512 row lanes, 4096 rows)
SHAPES = [(1, 4), (2, 12), (15, 20), (16, 4), (17, 36), (63, 12), (64, 68), (65, 20), (511, 12), (512, 36), (513, 68), (1023, 20),
          (1025, 100), (4095, 12), (4096, 68),
          (4097, 12), (4160, 36), (4161, 68), (8193, 20), (32768, 12), (32769, 36), (40961, 68),
          (700, 256), (5000, 64)]
CPU_SHAPES = [s for s in SHAPES if s[0] <= 8193]
F4, F8, LD = np.float32, np.float64, np.longdouble


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def columns(kind, n, c, g):
    """-> (x float32 [n, c], per-column scale of the output gradient [c]).  g: numpy Generator."""
    z = g.standard_normal((n, c))
    if kind == "scales":          # std over six decades, |mean| / std over four; column 0 constant
        std = 10.0 ** g.uniform(-3, 3, c)
        mean = std * 10.0 ** g.uniform(-2, 2, c) * g.choice([-1.0, 1.0], c)
        x = z * std + mean
        x[:, 0] = 3.25
    elif kind == "offset":        # std 1, mean 2^k: E[x^2] / var up to 2^24
        x = z + 2.0 ** (np.arange(c) % 13)
    else:                         # what test_gpu_dense.py uses: the same affine map for every column
        assert kind == "plain"
        x = z * 2.5 + 0.7
    return x.astype(F4), (10.0 ** g.uniform(-3, 3, c)).astype(F4)


def _colsum(a):
    return np.asarray(np.sum(a, axis=0, dtype=LD), dtype=F8)


def reference(x, gamma, beta, eps, residual, relu, gys, training, mean=None, var=None, momentum=None, rm=None, rv=None):
    """float64 elementwise, long-double column sums, two-pass variance.  -> namespace with y, mean, var, rm, rv (updated running
    buffers, training with buffers only), gx, gres, ggamma, gbeta (gys given only) and the magnitudes limits() needs.  The backward
    pass uses this reference's own ReLU mask."""
    r = types.SimpleNamespace(n=x.shape[0], relu=bool(relu), training=bool(training), nsrc=len(gys) if gys else 0)
    n = r.n
    x8 = x.astype(F8)
    r.ga, r.be = gamma.astype(F8), beta.astype(F8)
    e = F8(F4(eps))
    if training:
        m0 = _colsum(x8) / n
        d = x8 - m0
        sd = _colsum(d)
        r.mean = m0 + sd / n
        d = d - sd / n
        r.var = np.maximum(_colsum(d * d) / n, 0.0)
        r.ex2 = _colsum(x8 * x8) / n
        r.dv = C64 * r.ex2 / (r.var + e)
        if rm is not None:
            mom = F8(F4(momentum))
            r.unb = r.var * n / (n - 1) if n > 1 else r.var
            r.rm_in, r.rv_in, r.mom = rm.astype(F8), rv.astype(F8), mom
            r.rm = (1 - mom) * r.rm_in + mom * r.mean
            r.rv = (1 - mom) * r.rv_in + mom * r.unb
        else:
            r.rm = r.rv = None
    else:
        r.mean, r.var = mean.astype(F8), var.astype(F8)
        d = x8 - r.mean
        r.ex2 = None
        r.dv = np.zeros(x.shape[1])
        r.rm = r.rv = None
    r.is_ = 1.0 / np.sqrt(r.var + e)
    r.xhat = d * r.is_
    r.t = r.ga * r.xhat
    r.res = residual.astype(F8) if residual is not None else None
    r.pre = r.t + r.be + (r.res if r.res is not None else 0.0)
    r.y = np.maximum(r.pre, 0.0) if relu else r.pre
    return with_sources(r, gys) if gys else r


def with_sources(r, gys):
    """A copy of a reference() result with the backward pass under the gradient sources `gys` (the forward arrays are shared)."""
    r = copy.copy(r)
    r.nsrc = len(gys)
    n, relu, training = r.n, r.relu, r.training
    g = np.zeros_like(r.pre)
    r.gabs = np.zeros_like(r.pre)
    for s in gys:
        g += s.astype(F8)
        r.gabs += np.abs(s.astype(F8))
    if relu:
        keep = r.pre > 0
        g = np.where(keep, g, 0.0)
        r.gabs = np.where(keep, r.gabs, 0.0)
    r.g = r.gres = g
    r.gbeta = _colsum(g)
    r.ggamma = _colsum(g * r.xhat)
    k = r.ga * r.is_
    r.gx = k * (g - r.gbeta / n - r.xhat * r.ggamma / n) if training else k * g
    return r


def limits(r):
    """The limits of the module docstring for a reference() result -> namespace of arrays shaped like the quantities, plus
    `unclear` [n, c] and `excluded` [c] (columns left out of the backward checks)."""
    L = types.SimpleNamespace()
    n = r.n
    at, ax = np.abs(r.t), np.abs(r.xhat)
    ism = np.abs(r.is_ * r.mean)
    L.y = U * (16 * at + 2 * np.abs(r.ga) * ism + 4 * np.abs(r.be) + (4 * np.abs(r.res) if r.res is not None else 0.0)
               + 4 * np.abs(r.pre)) + at * r.dv + FLOOR
    L.unclear = (np.abs(r.pre) <= L.y) if r.relu else np.zeros(r.pre.shape, dtype=bool)
    L.excluded = L.unclear.any(0)
    if r.training:
        L.mean = 2 * U * np.abs(r.mean) + FLOOR
        L.var = 2 * U * r.var + C64 * r.ex2 + FLOOR
        if r.rm is not None:
            mom = r.mom
            L.rm = mom * L.mean + U * (4 * np.abs((1 - mom) * r.rm_in) + 2 * np.abs(mom * r.mean) + 2 * np.abs(r.rm)) + FLOOR
            L.rv = mom * (n / (n - 1) if n > 1 else 1.0) * L.var + U * (4 * np.abs((1 - mom) * r.rv_in) + 2 * np.abs(mom * r.unb)
                                                                         + 2 * np.abs(r.rv)) + FLOOR
    if not r.nsrc:
        return L
    ag = np.abs(r.g)
    dg = (r.nsrc - 1) * U * r.gabs
    dxh = U * (3 * ax + ism) + ax * r.dv
    L.gres = (r.nsrc * U * r.gabs + FLOOR) if r.nsrc > 1 else np.zeros_like(ag)
    L.gbeta = 2 * U * np.abs(r.gbeta) + 2.0 ** -49 * _colsum(ag) + _colsum(dg) + FLOOR
    L.ggamma = 2 * U * np.abs(r.ggamma) + 2 * _colsum(ag * dxh) + 2.0 ** -49 * _colsum(ag * ax) + _colsum(dg * ax) + FLOOR
    k = np.abs(r.ga * r.is_)
    if r.training:
        L.gx = ((16 * U + r.dv) * k * (ag + np.abs(r.gbeta) / n + np.abs(r.xhat * r.ggamma) / n)
                + 2 * k * (dxh * np.abs(r.ggamma) / n + ax * _colsum(dxh * ag) / n)
                + 2 * k * (dg + _colsum(dg) / n + ax * _colsum(dg * ax) / n) + FLOOR)
    else:
        L.gx = 16 * U * k * ag + 2 * k * dg + FLOOR
    return L


FORWARD = ("y", "mean", "var", "rm", "rv")
BACKWARD = ("gx", "gres", "ggamma", "gbeta")


def ratios(got, r, L):
    """{quantity: (worst err / limit, elements beyond the limit)} for the quantities present in `got` (name -> float32 array).
    Backward quantities are compared in the columns that are not excluded; gres with a zero limit must be equal."""
    out = {}
    for name in FORWARD + BACKWARD:
        if got.get(name) is None or getattr(r, name, None) is None:
            continue
        want, lim = getattr(r, name), getattr(L, name)
        have = np.asarray(got[name], dtype=F8)
        assert have.shape == want.shape, (name, have.shape, want.shape)
        if name in BACKWARD:
            keep = ~L.excluded
            have, want, lim = have[..., keep], want[..., keep], lim[..., keep]
        err = np.abs(have - want)
        bad = ~(err <= lim)                                            # (a NaN is beyond every limit)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / lim)
        out[name] = (float(np.nan_to_num(q, nan=np.inf).max()) if q.size else 0.0, int(bad.sum()))
    return out


def within(got, r, L, label, worst=None):
    """Assert every limit; -> {quantity: worst ratio}, and folds them into `worst` (a dict of running maxima) when given."""
    res = ratios(got, r, L)
    flat = {k: v[0] for k, v in res.items()}
    if worst is not None:
        for k, v in flat.items():
            worst[k] = max(worst.get(k, 0.0), v)
    bad = {k: v for k, v in res.items() if v[1]}
    assert not bad, "%s: beyond the limit (worst ratio, elements): %s" % (label, bad)
    return flat


def _sum64(a, acc=F8):
    """Column sums in float64 as a tree of fan-in 8: the depth of the kernels' own trees (a few rows per lane, 16 row lanes, 8 x 8 x 8
    partial blocks; or 8 rows per lane, 32 lanes, 16 waves), not a chain of n additions."""
    a = a.astype(acc)
    while a.shape[0] > 1:
        pad = -a.shape[0] % 8
        if pad:
            a = np.concatenate([a, np.zeros((pad,) + a.shape[1:], dtype=acc)])
        a = a.reshape(-1, 8, *a.shape[1:]).sum(1)
    return (a[0] if a.shape[0] else np.zeros(a.shape[1:])).astype(F8)


def emulate(x, gamma, beta, eps, residual, relu, gys, training, mean=None, var=None, momentum=None, rm=None, rv=None, mutant=None):
    """The kernels' arithmetic in numpy (module docstring) -> {name: float32 array}.  The fma is computed in float64 (the product of
    two fp32 values is exact there) and rounded once.  mutant: one of MUTANTS, the same arithmetic with that one defect:
      a  fp32 accumulators for the column sums of x and x^2         b  variance against the fp32-rounded mean
      c  the biased variance written to running_var                 d  the last n % 16 rows left out of the sums
      e  the last 4 columns take column 0's sums                    f  1 / (n - 1) instead of 1 / n in gx
      g  one block of 64 rows left out of the backward sums"""
    assert mutant is None or mutant in MUTANTS
    n, c = x.shape
    out = {}
    epsf = F4(eps)
    if training:
        xs = x[:n - n % 16] if mutant == "d" else x
        if mutant == "a":
            s1 = _sum64(xs, F4)
            s2 = _sum64(xs * xs, F4)
        else:
            s1 = _sum64(xs)
            s2 = _sum64(xs.astype(F8) ** 2)
        if mutant == "e" and c > 4:
            s1[-4:] = s1[0]
            s2[-4:] = s2[0]
        m = s1 / F8(n)
        mm = m.astype(F4).astype(F8) if mutant == "b" else m
        v = np.maximum(s2 / F8(n) - mm * mm, 0.0)
        mu, vr = m.astype(F4), v.astype(F4)
        out["mean"], out["var"] = mu, vr
        if rm is not None:
            mom = F4(momentum)
            one = F4(1) - mom
            unb = v * F8(n) / F8(n - 1) if (n > 1 and mutant != "c") else v
            out["rm"] = one * rm + mom * mu
            out["rv"] = one * rv + mom * unb.astype(F4)
    else:
        mu, vr = mean, var
    is_ = F4(1) / np.sqrt(vr + epsf)
    xh = (x - mu) * is_
    o = (xh.astype(F8) * gamma.astype(F8) + beta.astype(F8)).astype(F4)
    if residual is not None:
        o = o + residual
    if relu:
        o = np.where(o > 0, o, np.where(np.isnan(o), o, F4(0)))
    out["y"] = o
    assert o.dtype == F4 and is_.dtype == F4 and xh.dtype == F4
    if not gys:
        return out
    g = gys[0].copy()
    for s in gys[1:]:
        g = g + s
    if relu:
        g = np.where(o > 0, g, F4(0))
    out["gres"] = g
    rows = np.ones(n, dtype=bool)
    if mutant == "g" and n >= 64:
        b = 64 if n >= 128 else 0
        rows[b:b + 64] = False
    s1 = _sum64(g[rows])
    s2 = _sum64(g[rows].astype(F8) * xh[rows].astype(F8))
    sg, sx = s1.astype(F4), s2.astype(F4)
    out["gbeta"], out["ggamma"] = sg, sx
    k = gamma * is_
    if training:
        inv_n = F4(1) / F4(n - 1 if (mutant == "f" and n > 1) else n)
        gx = k * (g - sg * inv_n - xh * sx * inv_n)
    else:
        gx = k * g
    assert gx.dtype == F4
    out["gx"] = gx
    return out


def tensor_max_check(got, r):
    """Would the checks of test_gpu_dense.py (max |err| / max |ref| over the whole tensor, thresholds as there) pass `got`?"""
    tol = {"y": 2e-5, "gx": 5e-5, "ggamma": 5e-5, "gbeta": 5e-5, "gres": 2e-6, "rm": 1e-5, "rv": 1e-5}
    for name, t in tol.items():
        if got.get(name) is None or getattr(r, name, None) is None:
            continue
        want = getattr(r, name)
        rel = np.abs(np.asarray(got[name], dtype=F8) - want).max() / (np.abs(want).max() + 1e-30)
        if not rel < t:
            return False
    return True


# ---------------------------------------------------------------------------------------------------------------- the cases
# One case = the inputs of four configurations on the same x:
#   "plain"  training, no residual, no ReLU            "res"   training, residual + ReLU (gradient sources with gres)
#   "mask"   training, ReLU without a residual (the mask can be recomputed from x)
#   "eval"   evaluation mode (mean / var = the running buffers), residual + ReLU
Case = collections.namedtuple("Case", "kind n c x gamma beta res res_eval wide gys rm rv")
CONFIGS = ("plain", "res", "mask", "eval")


def config_args(case, config, nsrc=3):
    """Keyword arguments of reference() / emulate() for one configuration of a case."""
    training = config != "eval"
    a = dict(x=case.x, gamma=case.gamma, beta=case.beta, eps=EPS, relu=config != "plain", gys=list(case.gys[:nsrc]) if nsrc else None,
             residual={"plain": None, "res": case.res, "mask": None, "eval": case.res_eval}[config], training=training)
    if training:
        a.update(momentum=MOMENTUM, rm=case.rm, rv=case.rv)
    else:
        a.update(mean=case.rm, var=case.rv)
    return a


def _push_away(case_args, move, keep_constant=False, margin=4.0, rounds=8):
    """Move the pre-activations of a ReLU configuration away from zero: while an element lies within `margin` limits of zero,
    move(ref, lim, bad) changes the inputs in place.  (The test's condition is one limit; the margin is for the design.)"""
    for _ in range(rounds):
        r = reference(**dict(case_args, gys=None, rm=None, rv=None))
        L = limits(r)
        bad = np.abs(r.pre) <= margin * L.y
        if keep_constant:
            bad[:, r.var == 0] = False             # moving x: a constant column stays constant (its pre-activation is beta)
        if not bad.any():
            return
        move(r, L, bad)
    raise AssertionError("pre-activations could not be moved away from zero")


@functools.lru_cache(maxsize=3)
def case(kind, n, c):
    """The inputs of a case (shared, never modified after construction)."""
    g = np.random.default_rng(_seed("bn", kind, n, c))
    x, gscale = columns(kind, n, c, g)
    gamma = (g.uniform(0.5, 1.5, c) * np.where(g.random(c) < 0.25, -1.0, 1.0)).astype(F4)
    beta = (g.uniform(0.1, 0.5, c) * g.choice([-1.0, 1.0], c)).astype(F4)
    res = g.standard_normal((n, c)).astype(F4)
    res_eval = g.standard_normal((n, c)).astype(F4)
    wscale = np.concatenate([10.0 ** g.uniform(-3, 3, 8), gscale, 10.0 ** g.uniform(-3, 3, 16)])
    wide = (g.standard_normal((n, c + 24)) * wscale).astype(F4)           # source 0 is columns [8, 8 + c) of this
    gys = (wide[:, 8:8 + c], (g.standard_normal((n, c)) * gscale).astype(F4), (g.standard_normal((n, c)) * gscale).astype(F4))
    cm, cv = x.astype(F8).mean(0), x.astype(F8).var(0)
    rm = (cm * (1 + 0.1 * g.standard_normal(c))).astype(F4)
    rv = (cv * g.uniform(0.5, 2.0, c)).astype(F4)
    cs = Case(kind, n, c, x, gamma, beta, res, res_eval, wide, gys, rm, rv)

    def move_x(r, L, bad):
        step = np.maximum(16 * L.y / np.abs(r.ga * r.is_), 4 * np.spacing(np.abs(x)).astype(F8))
        x[bad] = (x.astype(F8) + np.where(r.pre >= 0, 1.0, -1.0) * np.sign(r.ga) * step)[bad].astype(F4)

    def move_res(which):
        def move(r, L, bad):
            which[bad] = (which.astype(F8) + np.where(r.pre >= 0, 1.0, -1.0) * 16 * L.y)[bad].astype(F4)
        return move

    _push_away(config_args(cs, "mask"), move_x, keep_constant=True)
    _push_away(config_args(cs, "res"), move_res(res))
    _push_away(config_args(cs, "eval"), move_res(res_eval))
    for a in (x, gamma, beta, res, res_eval, wide, rm, rv, gys[1], gys[2]):
        a.setflags(write=False)
    return cs
