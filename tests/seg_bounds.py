"""The arithmetic contract of the supervised head in one place (plain helper module; imported by test_seg_bounds_cpu.py and
test_gpu_seg_bounds.py): a float64 / long-double reference of the cross-entropy of csrc/seg.hip, per-row and per-element limits
derived from the roundings of the kernels' own expressions, a numpy emulation of that arithmetic, the emulation with one defect at a
time (MUTANTS); and the same for ONE step of osn_sgd_step / osn_adam_step (csrc/optim.hip).

Kernel arithmetic (csrc/seg.hip), x = one row of c fp32 logits, y its label.  A row lives in a group of G lanes, G = seg_group(c)
(seg.hip:213-215); lane g holds columns g, g + G, .., g + 7 G.  (m, bi) = the row maximum and its column by seg_better (seg.hip:30-34:
NaN is the largest value, the lowest column wins a tie).  Each lane adds expf(x_k - m) over ITS columns k != bi left to right (the
first sum adds to 0 and is exact), the G lane sums are added by the xor butterfly G / 2, .., 1 -> s1 (seg.hip:61-67); s1 = NaN when
m is not finite (seg.hip:71: such a row has no softmax; not part of the limits, see test_gpu_seg_bounds.py).  Forward:
val = (m - x_y) + log1pf(s1) in fp32 (seg.hip:117), added in fp64 per thread, per workgroup and over the workgroups
(seg_grid(n, c) = min(512, ceil(n / RPI)) of them, RPI = 256 / G rows per trip of the grid-stride loop, seg.hip:103,217-220);
loss = float(sum / double(n_valid)) (seg.hip:149,159).  Backward (seg.hip:171,185-193): sc = up / float(n_valid), inv = 1 / (1 + s1),
p_k = expf(x_k - m) * inv - [k == y] for k != bi;  p_bi = inv, or -s1 * inv when y == bi (1 / (1 + s1) - 1 without the cancellation);
g_k = sc * p_k.  Rows whose label is ignore_index or outside [0, c): +0.

Reference: the same quantities from the fp32 inputs, elementwise in float64 and row sums in long double, with the term of the
argmax kept out of s1 as the kernel has it: val_j = (m - x_y) + log1p(s1), loss = sum val_j / n_valid, softmax_k = exp(x_k - m) /
(1 + s1), gradient s (softmax - onehot) with s = up / n_valid and the argmax element as -s1 / (1 + s1) or 1 / (1 + s1).  The argmax
is decided on the fp32 inputs by the rules of seg_better, so no compared quantity depends on a decision the two precisions could take
differently, and no row has to be excluded (check_inputs: finite, no denormal element, no denormal difference x_k - m).

Limits, u = 2^-24 (one fp32 rounding; the quotient is correctly rounded in the project's build), every constant TWICE the first-order
count of roundings on the path.  A library function that is W ulps off counts as 2 W roundings (one ulp is at most 2 u of the result):

  E_EXP = E_LOG1P = 2 by the rule "twice the measured worst, rounded up to an integer, at least 2".  Measured with
  tools/probe_libm.hip on an MI355X (gfx950, HIP 7.2.26015, the project's compile flags) against the host's long double:
      expf    6.8 M arguments in [-104, 0]                       worst 0.8512 ulp (at -61.1053734)   -> ceil(1.70) = 2
              results below 2^-126 are NOT flushed: worst 1.0 x 2^-149
      log1pf  8.4 M arguments in [0, 255]                        worst 0.5599 ulp (at 0.333435059)
              2.1 M on a logarithmic grid 1e-30 .. 1             worst 0.5618 ulp (at 0.371574134)   -> ceil(1.12) = 2

  one term   e_k = expf(fl(x_k - m)):  E_EXP + |x_k - m| relative roundings (the rounded argument moves exp by |x_k - m| u).
  row sum    q_s(c) = (ceil(c / G) - 1) + log2 G roundings, the lane's left-to-right sum and the butterfly; every term is
             non-negative, so they are relative:  |s1_c - s1| <= u D1,  D1 = (q_s + E_EXP) s1 + T,  T = sum_{k != bi} |x_k - m| e_k.
  row loss   |err val| <= 2 u ((m - x_y)  [the difference]  + E_LOG1P log1p(s1)  + D1 / (1 + s1)  [s1's error through log1p]
             + val  [the final sum of two non-negative terms])
  mean loss  u |loss| (the one fp32 rounding of the result; the fp64 sums add 2^-53-sized terms) + the mean of the row limits.
  gradient, k != bi:   2 u |s| ((E_EXP + |x_k - m| + D1 / (1 + s1) + 2 + 1) softmax_k + 3 |p_k|): everything upstream of the
             subtraction -- the term, s1 inside inv, the sum 1 + s1, the quotient, the product -- is relative to softmax_k;  the
             subtraction, sc and the product with sc are relative to |p_k|.
  gradient, k == bi != y:  p = 1 / (1 + s1):   2 u |s| (D1 / (1 + s1) + 2 + 2) |p|.
  gradient, k == bi == y:  p = -s1 / (1 + s1), d p / d s1 = -1 / (1 + s1)^2:   2 u |s| (D1 / (1 + s1)^2 + (2 + 1 + 2) |p|); both parts
             are relative to |p| itself (D1 is a multiple of s1), which can be 1e-30: this is what sees `inv - 1.f` there.
  ignored rows and rows with a label outside [0, c):  bitwise +0.
  Every limit has the absolute floor FLOOR = 1e-37, at the denormal edge: an exp below 2^-126 carries an absolute error (measured: one
  unit of 2^-149; at most 255 terms, 4e-43), and a product below 2^-126 is rounded absolutely (2^-150).

Inputs (rows()): gauss (4 randn, what test_gpu_seg.py uses), confident (one column raised by 5 .. 150, log-uniform, the label on it for 80 % of
the rows: s1 from 1e-2 to below the underflow of exp), big (rows around +-1e4), ties (small integers: the lowest column must win and
the excluded term is well defined), wide (x_k - m down to -104, past the underflow edge of exp near -87).  About 15 % of the labels
are ignore_index: 255, or -100 when 255 is a class.

One optimizer step (csrc/optim.hip:24-31, 77-85), reference in float64 from the fp32 state and the fp32 values of the
hyper-parameters the kernel receives; the limit of every output element is twice the first-order error, each rounding weighted by the
magnitude of ITS result (sgd_step() / adam_step() carry the error along with the value; contracting a * b + c into an fma only
removes one of the counted roundings):
  d = g + wd p:                 u (|wd p| + |d|)
  buf' = mom buf + omd d:       u (|mom buf| + |omd d| + |buf'|) + |omd| err d           (first step: buf' = d)
  d' = d + mom buf' (Nesterov): err d + |mom| err buf' + u (|mom buf'| + |d'|)            (otherwise d' = buf')
  p' = p - lr d':               |lr| err d' + u (|lr d'| + |p'|)
  m' = m + c1 (d - m):          |c1| (err d + u |d - m|) + u |c1 (d - m)| + u |m'|        (c1 = 1 - beta1, exact in fp32)
  v' = b2 v + (c2 d) d:         u (|b2 v| + 2 |c2 d d| + |v'|) + 2 |c2 d| err d
  den = sqrtf(v') / bc2s + eps: err v' / (2 sqrt v' bc2s) + u (2 sqrt v' / bc2s + |den|)
  p' = p - (ss m') / den:       (|ss| err m' + 2 u |ss m'|) / den + |quo| err den / den + u |quo| + u |p'|      (ss = lr / bc1)
"""
import collections
import functools
import math
import types
import zlib

import numpy as np

U = 2.0 ** -24
FLOOR = 1e-37
E_EXP = 2
E_LOG1P = 2
MEASURED = {"expf": 0.8512, "log1pf": 0.5618, "rocm": "HIP 7.2.26015, gfx950"}          # ulps, tools/probe_libm.hip
assert E_EXP == max(2, math.ceil(2 * MEASURED["expf"])) and E_LOG1P == max(2, math.ceil(2 * MEASURED["log1pf"]))
F4, F8, LD = np.float32, np.float64, np.longdouble
KINDS = ("gauss", "confident", "big", "ties", "wide")
UPS = (1.0, 2.5, -0.75)
MUTANTS = ("a", "b", "c", "d", "e", "f", "g", "h", "i")
SEG_PER, SEG_THREADS, SEG_MAX_WG, SEG_HIST_MAX_C = 8, 256, 512, 90                     # seg.hip:17-20
C_ROWS = 37
C_SHAPES = [(C_ROWS, c) for c in (1, 2, 8, 9, 16, 17, 20, 21, 32, 33, 64, 65, 128, 129, 160, 256)]
N_CLASSES = (8, 20, 129)                                                             # G = 1, 4, 32


def seg_group(c):
    """seg.hip:213-215"""
    return 1 if c <= 8 else 2 if c <= 16 else 4 if c <= 32 else 8 if c <= 64 else 16 if c <= 128 else 32


def seg_grid(n, c):
    """seg.hip:217-220"""
    return max(1, min(SEG_MAX_WG, -(-n // (SEG_THREADS // seg_group(c)))))


def q_s(c):
    """The roundings one term passes on its way into s1 (module docstring)."""
    g = seg_group(c)
    return (-(-c // g) - 1) + int(math.log2(g))


def n_shapes(c):
    rpi = SEG_THREADS // seg_group(c)
    return [(n, c) for n in (1, rpi - 1, rpi, rpi + 1, 255 * rpi, 256 * rpi, 257 * rpi, 512 * rpi - 1, 512 * rpi + 1, 1024 * rpi + 3)]


N_SHAPES = [s for c in N_CLASSES for s in n_shapes(c)]
N_KINDS = ("gauss", "confident")
# loss and gradient (up = 2.5) of these cases were recorded from the build BEFORE the non-finite fix: tests/golden/seg_parent_bits.npz
PARENT_CASES = [("gauss", 37, 20), ("confident", 37, 160)]


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def ignore_of(c):
    return 255 if c <= 255 else -100


def rows(kind, n, c, g):
    """-> (x float32 [n, c], y int64 [n]) with about 15 % of the labels at ignore_of(c).  g: numpy Generator."""
    y = g.integers(0, c, n)
    if kind == "gauss":
        x = 4.0 * g.standard_normal((n, c))
    elif kind == "confident":
        x = g.standard_normal((n, c))
        col = g.integers(0, c, n)
        x[np.arange(n), col] += np.exp(g.uniform(np.log(5.0), np.log(150.0), n))            # log-uniform in [5, 150]
        y = np.where(g.random(n) < 0.8, col, y)
    elif kind == "big":
        x = np.where(g.random((n, 1)) < 0.5, -1e4, 1e4) + 3.0 * g.standard_normal((n, c))
    elif kind == "ties":
        x = g.integers(-2, 3, (n, c)).astype(F8)
    else:
        assert kind == "wide"
        x = -g.uniform(0.0, 104.0, (n, c)) + g.uniform(-50.0, 50.0, (n, 1))
        x[np.arange(n), g.integers(0, c, n)] += g.uniform(0.0, 10.0, n)
    y = np.where(g.random(n) < 0.15, ignore_of(c), y).astype(np.int64)
    x = x.astype(F4)
    check_inputs(x)
    return x, y


def check_inputs(x):
    """The conditions on the inputs: finite, no denormal element, no denormal difference x_k - m; and the argmax the float64
    reference takes is the one seg_better takes on the fp32 values (the lowest column among the largest)."""
    tiny = np.finfo(F4).tiny
    assert x.dtype == F4 and np.isfinite(x).all()
    assert ((x == 0) | (np.abs(x) >= tiny)).all(), "a denormal element"
    bi = np.argmax(x, axis=1)
    m = x[np.arange(x.shape[0]), bi]
    d = x - m[:, None]
    assert (d <= 0).all() and ((d == 0) | (d <= -tiny)).all(), "a denormal difference"
    first = np.argmax(x.astype(F8) == m.astype(F8)[:, None], axis=1)
    assert np.array_equal(first, bi) and np.array_equal(np.argmax(x.astype(F8), axis=1), bi)


Case = collections.namedtuple("Case", "kind n c x y ignore")


@functools.lru_cache(maxsize=6)
def case(kind, n, c):
    """The inputs of a case (shared, never modified)."""
    x, y = rows(kind, n, c, np.random.default_rng(_seed("seg", kind, n, c)))
    x.setflags(write=False)
    y.setflags(write=False)
    return Case(kind, n, c, x, y, ignore_of(c))


def _rowsum(a):
    return np.asarray(np.sum(a.astype(LD), axis=1), dtype=F8)


def reference(x, y, ignore, up=1.0):
    """float64 elementwise, long-double row sums -> namespace: loss, val [n] (the row losses, whatever the label's validity: 0 where
    it is not valid), grad [n, c], valid [n], pred [n] and the magnitudes limits() needs."""
    n, c = x.shape
    ar = np.arange(n)
    r = types.SimpleNamespace(n=n, c=c, up=float(F4(up)))
    v = x.astype(F8)
    r.pred = bi = np.argmax(x, axis=1)
    r.valid = valid = (y != ignore) & (y >= 0) & (y < c)
    r.n_valid = nv = int(valid.sum())
    yy = np.where(valid, y, 0)
    m = v[ar, bi]
    r.dist = np.abs(v - m[:, None])
    e = np.exp(-r.dist)
    e[ar, bi] = 0.0
    r.s1 = s1 = _rowsum(e)
    with np.errstate(invalid="ignore"):
        r.T = _rowsum(np.where(e > 0, r.dist * e, 0.0))                  # (a -inf logit: exp = 0, no term)
    r.gap = np.where(valid, m - v[ar, yy], 0.0)
    r.l1p = np.log1p(s1)
    r.val = np.where(valid, r.gap + r.l1p, 0.0)
    r.loss = float(np.sum(r.val[valid].astype(LD)) / nv) if nv else float("nan")
    r.s = r.up / nv if nv else 0.0
    r.soft = e / (1.0 + s1)[:, None]
    r.soft[ar, bi] = 1.0 / (1.0 + s1)
    p = r.soft.copy()
    p[ar, yy] -= 1.0
    r.on_arg = on = valid & (yy == bi)
    p[ar[on], bi[on]] = -(s1 / (1.0 + s1))[on]
    p[~valid] = 0.0
    r.p = p
    r.grad = r.s * p
    return r


def limits(r):
    """The limits of the module docstring -> namespace: val [n] (row losses), loss (scalar), grad [n, c] (0 on rows without a valid
    label: those are compared bit by bit)."""
    L = types.SimpleNamespace()
    ar = np.arange(r.n)
    D1 = (q_s(r.c) + E_EXP) * r.s1 + r.T
    r1 = D1 / (1.0 + r.s1)
    L.val = 2 * U * (r.gap + E_LOG1P * r.l1p + r1 + r.val) + FLOOR
    L.loss = (U * abs(r.loss) + float(np.mean(L.val[r.valid]))) if r.n_valid else 0.0
    with np.errstate(invalid="ignore"):
        cnt = np.where(r.soft > 0, ((E_EXP + 3) + r.dist + r1[:, None]) * r.soft, 0.0) + 3 * np.abs(r.p)
    arg = np.where(r.on_arg, D1 / (1.0 + r.s1) ** 2 + 5 * np.abs(r.p[ar, r.pred]), (r1 + 4) * np.abs(r.p[ar, r.pred]))
    cnt[ar, r.pred] = arg
    L.grad = np.where(r.valid[:, None], 2 * U * abs(r.s) * cnt + FLOOR, 0.0)
    return L


def _bits(a):
    return np.ascontiguousarray(a, dtype=F4).view(np.int32)


def _worst(err, lim):
    bad = ~(err <= lim)                                                  # (a NaN is beyond every limit)
    with np.errstate(divide="ignore", invalid="ignore"):
        qn = np.where(err == 0, 0.0, err / lim)
    qn = np.nan_to_num(qn, nan=np.inf)
    return (float(qn.max()) if qn.size else 0.0, int(bad.sum()))


def ratios(got, r, L):
    """{quantity: (worst err / limit, elements beyond the limit)} for got = {"loss": fp32 scalar, "grad": fp32 [n, c]} (either may be
    missing).  "zeros": the rows without a valid label, bit by bit."""
    res = {}
    if got.get("loss") is not None:
        if r.n_valid:
            res["loss"] = _worst(np.abs(np.array([float(got["loss"]) - r.loss])), np.array([L.loss]))
        else:
            res["loss"] = (0.0, 0) if np.isnan(got["loss"]) else (np.inf, 1)
    g = got.get("grad")
    if g is not None:
        g = np.asarray(g)
        assert g.shape == (r.n, r.c) and g.dtype == F4, (g.shape, g.dtype)
        nz = int(np.count_nonzero(_bits(g[~r.valid])))
        res["zeros"] = (np.inf if nz else 0.0, nz)
        res["grad"] = _worst(np.abs(g[r.valid].astype(F8) - r.grad[r.valid]), L.grad[r.valid])
    return res


def within(got, r, L, label, worst=None):
    """Assert every limit; -> {quantity: worst ratio}, folded into `worst` (a dict of running maxima) when given."""
    res = ratios(got, r, L)
    flat = {k: v[0] for k, v in res.items()}
    if worst is not None:
        for k, v in flat.items():
            worst[k] = max(worst.get(k, 0.0), v)
    bad = {k: v for k, v in res.items() if v[1]}
    assert not bad, "%s: beyond the limit (worst ratio, elements): %s" % (label, bad)
    return flat


def emulate(x, y, ignore, up=1.0, mutant=None):
    """The kernels' arithmetic in numpy, fp32 operation by operation in their order (module docstring; exp and log1p correctly
    rounded) -> {"loss": float32, "val": float32 [n], "grad": float32 [n, c]}.  mutant: one of MUTANTS, the same arithmetic with that
    one defect:
      a  p = inv - 1.f where the label is the argmax              b  logf(1.f + s1) for log1pf(s1)
      c  the upstream gradient ignored (sc = 1 / n_valid)         d  the butterfly started one step low (at G / 4)
      e  the 8th value of a lane dropped (c > 7 G)                f  the loss partials without the trips of the grid-stride loop
      g  sc = up / n, not up / n_valid                               past the first
      h  an ignored row's gradient left at sc softmax             i  seg_mean_kernel reading only the first 256 partials (sums
                                                                     and counts)"""
    assert mutant is None or mutant in MUTANTS
    n, c = x.shape
    G = seg_group(c)
    rpi, nb = SEG_THREADS // G, seg_grid(n, c)
    ar = np.arange(n)
    one = F4(1)
    bi = np.argmax(x, axis=1)
    m = x[ar, bi]
    valid = (y != ignore) & (y >= 0) & (y < c)
    yy = np.where(valid, y, 0)
    k = np.arange(SEG_PER * G)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        w = np.full((n, SEG_PER * G), -np.inf, dtype=F4)
        w[:, :c] = x
        e = np.exp((w - m[:, None]).astype(F8)).astype(F4)                         # expf(v - m); pads: expf(-inf) = 0
        live = np.where((k[None, :] < c) & (k[None, :] != bi[:, None]), e, F4(0)).reshape(n, SEG_PER, G)
        s = np.zeros((n, G), dtype=F4)
        for t in range(SEG_PER - (1 if mutant == "e" else 0)):
            s = s + live[:, t, :]
        lanes = np.arange(G)
        step = G // 4 if mutant == "d" else G // 2
        while step >= 1:
            s = s + s[:, lanes ^ step]
            step //= 2
        s1 = s[:, 0]
        assert s1.dtype == F4
        lg = np.log((one + s1).astype(F8)).astype(F4) if mutant == "b" else np.log1p(s1.astype(F8)).astype(F4)
        val = (m - x[ar, yy]) + lg
        blk = ar // rpi
        in_sum = valid & (blk // nb == 0) if mutant == "f" else valid
        counted = valid
        if mutant == "i":
            in_sum = in_sum & (blk % nb < 256)
            counted = valid & (blk % nb < 256)
        nv = int(counted.sum())
        loss = F4(np.sum(val[in_sum].astype(F8)) / F8(nv)) if nv else F4(np.nan)
        sc = (one if mutant == "c" else F4(up)) / F4(n if mutant == "g" else nv) if nv else F4(0)
        inv = one / (one + s1)
        soft = e[:, :c] * inv[:, None]
        hot = np.zeros((n, c), dtype=F4)
        hot[ar, yy] = 1
        p = soft - hot
        p[ar, bi] = np.where(yy == bi, (inv - one) if mutant == "a" else (-s1 * inv), inv)
        grad = sc * p
        if mutant == "h":
            soft[ar, bi] = inv
            grad[~valid] = (sc * soft)[~valid]
        else:
            grad[~valid] = 0
        assert val.dtype == F4 and grad.dtype == F4 and inv.dtype == F4
    return {"loss": loss, "val": np.where(valid, val, F4(0)), "grad": grad}


def old_check(got, r):
    """Would the criteria of test_gpu_seg.py::test_loss_and_gradient_against_torch_float64 pass `got` (computed at up = 1)?  The loss
    within 2e-6 of the float64 one, relative; the gradient within 1e-6 in the relative L2 norm of the whole matrix."""
    loss_ok = abs(float(got["loss"]) - r.loss) <= 2e-6 * abs(r.loss)
    g = np.asarray(got["grad"], dtype=F8)
    rel = np.linalg.norm(g - r.grad) / (np.linalg.norm(r.grad) + 1e-300)
    return bool(loss_ok and rel <= 1e-6)


OLD_SHAPES = [(1, 20), (7, 3), (5000, 21), (100999, 20), (20000, 160), (3000, 256)]    # of test_gpu_seg.py's SHAPES
OLD_SCALES = (1.0, 80.0)


def old_inputs(n, c, scale):
    """Inputs of the kind test_gpu_seg.py's make() draws: scale * randn, uniform labels, 15 % ignored."""
    g = np.random.default_rng(_seed("old", n, c, scale))
    x = (scale * g.standard_normal((n, c))).astype(F4)
    y = np.where(g.random(n) < 0.15, 255, g.integers(0, c, n)).astype(np.int64)
    return x, y, 255


# ------------------------------------------------------------------------------------------------ one optimizer step
SGD_SETTINGS = [dict(momentum=m, dampening=d, nesterov=ne, weight_decay=wd)
                for m in (0.0, 0.9) for d in (0.0, 0.1) for ne in (False, True) for wd in (0.0, 1e-4)
                if not (ne and (m == 0 or d != 0))]                                 # test_gpu_seg.py's SGD_SETTINGS
ADAM_SETTINGS = [dict(step=s, weight_decay=wd) for s in (1, 1000) for wd in (0.0, 0.01)]
OPT_SIZES = (4, 1020, 1024, 1028, 8192 * 256 * 4 + 4)                               # the last: one element group past the grid cap
OPT_FLOOR = 1e-37


def f32(v):
    return float(F4(v))


def sgd_step(p, g, buf, lr, momentum, dampening, weight_decay, nesterov, first):
    """One step of optim.hip:77-85 on float64 copies of the fp32 state (numpy arrays or torch tensors: only + - * abs are used)
    -> (p', buf' or None, limit of p', limit of buf' or None).  The hyper-parameters are the fp32 values the kernel receives."""
    lr, mom, wd = f32(lr), f32(momentum), f32(weight_decay)
    omd = f32(1.0 - float(dampening))
    d, ed = g, 0.0 * g
    if wd != 0.0:
        d = g + wd * p
        ed = U * (abs(wd * p) + abs(d))
    nbuf = ebuf = None
    if mom != 0.0:
        if first:
            nbuf, ebuf = d, ed
        else:
            nbuf = mom * buf + omd * d
            ebuf = U * (abs(mom * buf) + abs(omd * d) + abs(nbuf)) + abs(omd) * ed
        if nesterov:
            d2 = d + mom * nbuf
            ed = ed + abs(mom) * ebuf + U * (abs(mom * nbuf) + abs(d2))
            d = d2
        else:
            d, ed = nbuf, ebuf
    np_ = p - lr * d
    ep = abs(lr) * ed + U * (abs(lr * d) + abs(np_))
    return np_, nbuf, 2 * ep + OPT_FLOOR, (None if nbuf is None else 2 * ebuf + OPT_FLOOR)


def adam_step(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay):
    """One step of optim.hip:24-31 (bias corrections as osn_adam_step computes them, optim.hip:51-56) on float64 copies of the fp32
    state -> (p', m', v', limit p', limit m', limit v')."""
    lr, b1, b2, eps, wd = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(weight_decay)
    bc1 = f32(1.0 - b1 ** step)
    bc2s = f32(math.sqrt(1.0 - b2 ** step))
    c1, c2 = f32(1.0 - b1), f32(1.0 - b2)
    assert c1 == 1.0 - b1 and c2 == 1.0 - b2                                       # 1.f - beta is exact in fp32
    ss = lr / bc1
    d, ed = g, 0.0 * g
    if wd != 0.0:
        d = g + wd * p
        ed = U * (abs(wd * p) + abs(d))
    t = d - m
    nm = m + c1 * t
    em = c1 * (ed + U * abs(t)) + U * abs(c1 * t) + U * abs(nm)
    nv = b2 * v + c2 * d * d
    ev = U * (abs(b2 * v) + 2 * abs(c2 * d * d) + abs(nv)) + 2 * abs(c2 * d) * ed
    sq = nv ** 0.5
    den = sq / bc2s + eps
    eden = ev / (2 * sq * bc2s + 1e-300) + U * (2 * sq / bc2s + den)
    quo = ss * nm / den
    equo = (abs(ss) * em + 2 * U * abs(ss * nm)) / den + abs(quo) * eden / den + U * abs(quo)
    np_ = p - quo
    ep = equo + U * abs(np_)
    return np_, nm, nv, 2 * ep + OPT_FLOOR, 2 * em + OPT_FLOOR, 2 * ev + OPT_FLOOR


def opt_state(n, seed=0):
    """fp32 state for a flat buffer of n elements: parameters over six decades, a tenth of the gradients zero, moments of a plausible
    size (v >= 0, a tenth of them zero where the gradient is zero too).  numpy; deterministic."""
    g_ = np.random.default_rng(_seed("opt", n, seed))
    p = (g_.standard_normal(n) * 10.0 ** g_.uniform(-3, 3, n)).astype(F4)
    zero = g_.random(n) < 0.1
    g = np.where(zero, 0.0, g_.standard_normal(n) * 10.0 ** g_.uniform(-2, 1, n)).astype(F4)
    buf = (g_.standard_normal(n) * 10.0 ** g_.uniform(-2, 1, n)).astype(F4)
    v = np.where(zero, 0.0, g_.standard_normal(n) ** 2 * 10.0 ** g_.uniform(-4, 2, n)).astype(F4)
    return p, g, buf, v
