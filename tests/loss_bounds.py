"""The arithmetic contract of the distillation loss in one place (plain helper module; imported by test_loss_bounds_cpu.py and
test_gpu_loss_bounds.py): a float64 / long-double reference, per-element and per-loss limits derived from the roundings of the
kernels' own expressions, a numpy emulation of that arithmetic, and the emulation with one defect at a time (MUTANTS).

Kernel arithmetic (csrc/loss.hip), a = out[sel[j]], b = target[j], all fp32.  Forward, one wave per selected row: lane l adds
(x0 y0 + x1 y1) + x2 y2) + x3 y3 of columns 4l .. 4l+3 of each 256-column step to its accumulator, the 64 accumulators are summed
by the xor butterfly 32, 16, .., 1 -> dot, a2 = sum a^2, b2 = sum b^2;  na = max(sqrtf(a2), 1e-8f) (a NaN is kept), nb likewise;
val = 1 - dot / (na * nb);  L1: val = the same sum over |x - y|.  loss = float(sum_j double(val[j]) * scale), scale = 1 / n_sel
(1 / (n_sel d) for L1) in fp64.  Backward, one wave per OUTPUT row r with j = pos[r] (pos[sel[j]] = j, -1 elsewhere):
s = -up / float(n_sel);  kb = s / (na * nb);  ka = sqrtf(a2) > 1e-8f ? -s * dot / (na * na * na * nb) : 0;  g = kb * y + ka * x.
L1: s32 = up / (float(n_sel) * float(d)), g = +s32 / -s32 / 0 by the sign of the fp32 difference x - y.  Rows with pos[r] < 0: +0.

Reference: the same quantities in float64 on the fp32 inputs (a product of two fp32 values is exact there), row sums in long double;
dot, A = sum a^2, B = sum b^2, S = sum |a_i b_i|;  na = max(sqrt A, 1e-8), nb = max(sqrt B, 1e-8);  val_j = 1 - dot / (na nb);
gradient row s (b / (na nb) - [sqrt A > eps] dot a / (na^3 nb)), s = -up / n_sel.

Limits, u = 2^-24 (one fp32 rounding: sqrtf and the quotient are correctly rounded in the project's build), every constant TWICE
the first-order count of roundings on the path.

  q(d), the roundings one element passes on its way into a row sum:  1 (the product; for L1 the difference) + 3 (the four-term sum
  of a lane) + ceil(d / 256) - 1 (the lane's accumulations: the first one adds to 0 and is exact) + ceil(log2(min(64, d / 4)))
  (the butterfly steps in which both operands can be non-zero: lanes from d / 4 on hold 0).  q(4) = 4, q(20) = 7, q(256) = 10,
  q(768) = 12, q(1028) = 14.  So |dot_c - dot| <= q u S, and A, B carry a relative error q u.
  A norm: sqrt halves the relative error of its argument and rounds once: e_n = q / 2 + 1.  (A clamped norm is exact but for the fp32
  rounding of 1e-8 itself, 6e-9 = 0.1 u relative: inside e_n.)

  cosine gradient, element (j, i).  Write g = T1 - T2, T1 = s b_i / (na nb), T2 = s dot a_i / (na^3 nb), and T2' the same with S in
  the place of dot.  The computed s, na and nb are THE SAME numbers in kb and in ka, so their errors move T1 and T2 together and
  reach the result only in proportion to g itself, as does the rounding of the final sum:
      common to both terms      1 (s) + e_n (na) + e_n (nb) + 1 (the sum kb y + ka x)                             = q + 4    on |g|
      T1 alone                  1 (na * nb) + 1 (the quotient kb) + 1 (kb * y)                                    = 3        on |T1|
      T2 alone                  q (dot, relative to S) + 1 (s * dot) + 2 e_n (the two further factors na) + 3 (the products of
                                the denominator) + 1 (the quotient ka) + 1 (ka * x)                               = 2 q + 8  on |T2'|
      limit  =  2 u ((q + 4) |g| + 3 |T1| + (2 q + 8) |T2'|)                          (under the clamp sqrt A <= eps: T2 = T2' = 0)
  Since |g| <= |T1| + |T2'| this is everywhere at most  C_g u |s| (|b_i| + (S / A) |a_i|) / (na nb)  with C_g = 2 (3 q + 12), the
  single-constant form (limit_single(); test_loss_bounds_cpu.py asserts the inequality): who meets `limit` meets that one.  The
  split is what lets the limit see a wrong coefficient where it matters: on a row aligned with its target T1 and T2 cancel, g is
  tiny, and 2 (q + 4) u |g| does not hide an error of a few u in ka alone.

  cosine loss.  val_j:  q u S / (na nb) (dot) + (2 e_n + 1 + 1) u |cos| (na, nb, their product, the quotient) + u |val| (the
  difference);  |cos| <= S / (na nb) and |val| <= 1 + S / (na nb), so |err val_j| <= (2 q + 5) u (1 + S / (na nb)).  The fp64 sum and
  scale add 2^-53-sized terms; the result is rounded to fp32 once.
      limit  =  u |loss| + C_v u mean_j (1 + S_j / (na_j nb_j)),   C_v = 2 (2 q + 5)
  L1 loss: every term is non-negative, so the q roundings of a row sum and the final one are relative:
      limit  =  C_1 u loss,   C_1 = 2 (q + 1)
  L1 gradient: no limit -- bitwise +s32, -s32 or +0 (reference(): r.grad32).
  Rows outside sel: bitwise +0.  Every limit has the absolute floor 1e-37.

Inputs (rows()): no row norm within a factor 1 +- 1e-3 of eps, so the fp32 and the fp64 clamp decisions agree and no row has to be
excluded; every non-zero element a normal fp32 number.
"""
import collections
import functools
import math
import types
import zlib

import numpy as np

U = 2.0 ** -24
FLOOR = 1e-37
EPS = 1e-8
F4, F8, LD = np.float32, np.float64, np.longdouble
EPS32 = F4(1e-8)
KINDS = ("gauss", "aligned", "decades", "clamp")
LOSS_TYPES = ("cosine", "l1")
UPS = (1.0, 2.5, -0.75)
MUTANTS = ("a", "b", "c", "d", "e", "f", "g", "h")
# (n, n_sel, d).  d at the edges of `for (c = 4 * lane; c < d; c += 256)`, one lane (d = 4) to five steps; n_sel at the edges of the
# four rows per workgroup and of loss_mean_kernel's 1024 threads, with n = n_sel + 0, 1, 2, 3 in turn (n_sel == n: no compacted rows)
D_SHAPES = [(50, 37, d) for d in (4, 20, 252, 256, 260, 508, 512, 516, 768, 1024, 1028)]
N_SHAPES = [(n_sel + i % 4, n_sel, 20) for i, n_sel in enumerate((1, 3, 4, 5, 1023, 1024, 1025, 2049))]
SHAPES = D_SHAPES + N_SHAPES
SORTED_CASE = ("gauss", 50, 37, 260)              # the one case whose sel is sorted, as every selection of the older tests is
DENSE_SHAPES = [(5000, 1200, 768), (777, 777, 512), (64, 1, 20)]      # test_gpu_dense.py::test_distill_loss_forward_and_gradient
CLAMP_ROWS = 12                                   # kinds of degenerate row in the "clamp" inputs, see rows()


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def q_of(d):
    """The roundings one element passes on its way into a row sum (module docstring)."""
    return 4 + (-(-d // 256) - 1) + int(math.ceil(math.log2(min(64, d // 4))))


def _unit_fp16(g, n, d):
    """Unit rows rounded through fp16, as the fused features are."""
    z = g.standard_normal((n, d))
    return (z / np.linalg.norm(z, axis=1, keepdims=True)).astype(np.float16).astype(F4)


def _with_norm(g, d, norm):
    z = g.standard_normal(d)
    return (z / np.linalg.norm(z) * norm).astype(F4)


def rows(kind, n_sel, d, g, loss_type="cosine"):
    """-> (a, b) float32 [n_sel, d]: the selected output rows and their targets.  g: numpy Generator."""
    b = _unit_fp16(g, n_sel, d)
    if kind == "gauss":                  # what test_gpu_dense.py uses
        a = (2.5 * g.standard_normal((n_sel, d))).astype(F4)
    elif kind == "aligned":              # a = t b + noise: the two terms of the gradient cancel
        t = np.round(g.uniform(0.5, 20.0, n_sel) * 64) / 64              # (<= 11 significant bits: t b is exact in fp32 for an fp16 b)
        rel = 10.0 ** g.uniform(-5, -1, n_sel)
        scale = np.linalg.norm(b.astype(F8), axis=1) / np.sqrt(d)
        noise = (rel * t * scale)[:, None] * g.standard_normal((n_sel, d))
        j = np.arange(n_sel)
        noise[j % 10 == 0] = 0.0                                         # every tenth row exactly t b ...
        t = np.where(j % 20 == 10, -t, t)                                # ... and every other one of those exactly -t b
        a = (t[:, None] * b.astype(F8) + noise).astype(F4)
        assert np.array_equal(a[::10].astype(F8), t[::10, None] * b[::10].astype(F8))
    elif kind == "decades":              # column scales over six decades on the output, the reversed scales on the target
        sc = 10.0 ** g.uniform(-3, 3, d)
        a = (2.5 * g.standard_normal((n_sel, d)) * sc).astype(F4)
        b = (b.astype(F8) * sc[::-1]).astype(F4)
    else:                                # degenerate rows mixed into ordinary ones: row j with j % 3 == 0 takes kind (j // 3) % 12
        assert kind == "clamp"
        a = (2.5 * g.standard_normal((n_sel, d))).astype(F4)
        lo, hi = 0.5e-8, 2e-8
        table = [(0, None), (None, 0), (0, 0), (lo, None), (hi, None), (None, lo), (None, hi), (lo, lo), (lo, hi), (hi, lo), (hi, hi), (0, hi)]
        assert len(table) == CLAMP_ROWS
        for j in range(0, n_sel, 3):
            na, nb = table[(j // 3) % CLAMP_ROWS]
            if na is not None:
                a[j] = _with_norm(g, d, na) if na else 0
            if nb is not None:
                b[j] = _with_norm(g, d, nb) if nb else 0
    if loss_type == "l1":                # a tenth of the elements with a_i == b_i exactly
        assert kind == "gauss"
        same = g.random((n_sel, d)) < 0.1
        a[same] = b[same]
    check_inputs(a, b)
    return a, b


def check_inputs(a, b):
    """The conditions on the inputs: norms clear of the clamp, every non-zero element a normal fp32 number."""
    tiny = np.finfo(F4).tiny
    for x in (a, b):
        assert x.dtype == F4 and np.isfinite(x).all()
        assert ((x == 0) | (np.abs(x) >= tiny)).all(), "a denormal element"
        nrm = np.sqrt(np.asarray(np.sum(x.astype(LD) ** 2, axis=1), dtype=F8))
        assert not ((nrm > EPS * (1 - 1e-3)) & (nrm < EPS * (1 + 1e-3))).any(), "a row norm within 1e-3 of eps"
    sq = np.concatenate([(a.astype(F8) ** 2).ravel(), (b.astype(F8) ** 2).ravel(), np.abs(a.astype(F8) * b.astype(F8)).ravel()])
    assert ((sq == 0) | (sq >= tiny)).all(), "a product of two elements is denormal in fp32"


Case = collections.namedtuple("Case", "kind loss_type n n_sel d out sel target")


@functools.lru_cache(maxsize=8)
def case(kind, n, n_sel, d, loss_type="cosine", sort=False):
    """The inputs of a case (shared, never modified): out [n, d] with rows() at `sel` and Gaussian rows elsewhere; sel a sample of a
    random permutation, UNSORTED unless sort is set."""
    g = np.random.default_rng(_seed("loss", kind, n, n_sel, d, loss_type))
    a, b = rows(kind, n_sel, d, g, loss_type)
    out = (2.5 * g.standard_normal((n, d))).astype(F4)
    sel = g.permutation(n)[:n_sel].astype(np.int64)
    if sort:
        sel.sort()
    elif n_sel > 1 and (np.diff(sel) > 0).all():
        sel = sel[::-1].copy()                                           # (a short sample that came out in order)
    out[sel] = a
    for x in (out, sel, b):
        x.setflags(write=False)
    return Case(kind, loss_type, n, n_sel, d, out, sel, b)


def _rowsum(x):
    return np.asarray(np.sum(x.astype(LD), axis=1), dtype=F8)


def reference(out, sel, target, loss_type="cosine", up=1.0):
    """float64 elementwise, long-double row sums -> namespace with loss, val [n_sel], grad [n, d] (rows outside sel zero), keep [n]
    and the magnitudes limits() needs.  L1: also s32 and grad32, the gradient the kernel must produce bit by bit."""
    n, d = out.shape
    n_sel = sel.shape[0]
    a, b = out[sel].astype(F8), target.astype(F8)
    r = types.SimpleNamespace(loss_type=loss_type, n=n, n_sel=n_sel, d=d, sel=sel, up=float(F4(up)))
    r.keep = np.zeros(n, dtype=bool)
    r.keep[sel] = True
    r.grad = np.zeros((n, d))
    if loss_type == "cosine":
        r.dot, r.A, r.B, r.S = _rowsum(a * b), _rowsum(a * a), _rowsum(b * b), _rowsum(np.abs(a * b))
        r.live = np.sqrt(r.A) > EPS
        r.na, r.nb = np.maximum(np.sqrt(r.A), EPS), np.maximum(np.sqrt(r.B), EPS)
        r.val = 1.0 - r.dot / (r.na * r.nb)
        r.loss = float(np.sum(r.val.astype(LD)) / n_sel)
        r.s = -r.up / n_sel
        k = (r.s / (r.na * r.nb))[:, None]
        r.T1 = k * b
        r.T2 = np.where(r.live[:, None], k * (r.dot / r.na ** 2)[:, None] * a, 0.0)
        r.T2S = np.where(r.live[:, None], k * (r.S / r.na ** 2)[:, None] * a, 0.0)
        r.grows = r.T1 - r.T2
    else:
        assert loss_type == "l1"
        r.val = _rowsum(np.abs(a - b))
        r.loss = float(np.sum(r.val.astype(LD)) / (n_sel * d))
        r.grows = np.sign(a - b) * r.up / (n_sel * d)
        r.s32 = F4(up) / (F4(n_sel) * F4(d))
        diff = out[sel] - target                                          # the fp32 difference, whose sign the kernel takes
        r.grad32 = np.zeros((n, d), dtype=F4)
        r.grad32[sel] = np.where(diff > 0, r.s32, np.where(diff < 0, -r.s32, F4(0)))
    r.grad[sel] = r.grows
    return r


def limits(r):
    """The limits of the module docstring -> namespace: loss (scalar) and, for the cosine, grad [n, d] (0 outside sel: those rows are
    compared bit by bit)."""
    L = types.SimpleNamespace()
    q = q_of(r.d)
    if r.loss_type == "l1":
        L.loss = 2 * (q + 1) * U * abs(r.loss) + FLOOR
        return L
    L.loss = U * abs(r.loss) + 2 * (2 * q + 5) * U * float(np.mean(1.0 + r.S / (r.na * r.nb))) + FLOOR
    L.grad = np.zeros((r.n, r.d))
    L.grad[r.sel] = 2 * U * ((q + 4) * np.abs(r.grows) + 3 * np.abs(r.T1) + (2 * q + 8) * np.abs(r.T2S)) + FLOOR
    return L


def limit_single(r):
    """The single-constant form of the gradient limit, C_g u |s| (|b_i| + (S / A) |a_i|) / (na nb) with C_g = 2 (3 q + 12), on the
    selected rows [n_sel, d]: never below limits().grad there."""
    return 2 * (3 * q_of(r.d) + 12) * U * (np.abs(r.T1) + np.abs(r.T2S)) + FLOOR


def _bits(x):
    return np.ascontiguousarray(x, dtype=F4).view(np.int32)


def ratios(got, r, L):
    """{quantity: (worst err / limit, elements beyond the limit)} for got = {"loss": fp32 scalar, "grad": fp32 [n, d]} (either may
    be missing).  "zeros": the rows outside sel, bit by bit; the L1 gradient is compared bit by bit with r.grad32 ("grad": 0 or inf)."""
    res = {}
    if got.get("loss") is not None:
        err = abs(float(got["loss"]) - r.loss)
        res["loss"] = ((err / L.loss) if err == err else np.inf, int(not err <= L.loss))
    g = got.get("grad")
    if g is None:
        return res
    g = np.asarray(g)
    assert g.shape == (r.n, r.d) and g.dtype == F4, (g.shape, g.dtype)
    nz = int(np.count_nonzero(_bits(g[~r.keep])))
    res["zeros"] = (np.inf if nz else 0.0, nz)
    if r.loss_type == "l1":
        bad = int((_bits(g) != _bits(r.grad32)).sum())
        res["grad"] = (np.inf if bad else 0.0, bad)
        return res
    err = np.abs(g[r.sel].astype(F8) - r.grows)
    lim = L.grad[r.sel]
    bad = ~(err <= lim)                                                  # (a NaN is beyond every limit)
    with np.errstate(divide="ignore", invalid="ignore"):
        qn = np.where(err == 0, 0.0, err / lim)
    res["grad"] = (float(np.nan_to_num(qn, nan=np.inf).max()), int(bad.sum()))
    return res


def worst_ratio(got, r, L):
    return {k: v[0] for k, v in ratios(got, r, L).items()}


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


def _wave_sums(p, mutant=None):
    """Row sums of p float32 [rows, d] in the kernel's order: per 256-column step each of 64 lanes sums its four columns left to right,
    adds that to its accumulator; then the xor butterfly.  (Padding with +0 changes nothing: lanes past d hold 0.)"""
    rows_, d = p.shape
    steps = -(-d // 256)
    if mutant == "f" and d > 256 and d % 256:
        steps -= 1                                                       # the last, partial step never runs
    w = np.zeros((rows_, steps * 256), dtype=F4)
    m = min(d, steps * 256)
    w[:, :m] = p[:, :m]
    w = w.reshape(rows_, steps, 64, 4)
    acc = np.zeros((rows_, 64), dtype=F4)
    for k in range(steps):
        acc = acc + (((w[:, k, :, 0] + w[:, k, :, 1]) + w[:, k, :, 2]) + w[:, k, :, 3])
    lanes = np.arange(64)
    for m in ((16, 8, 4, 2, 1) if mutant == "e" else (32, 16, 8, 4, 2, 1)):
        acc = acc + acc[:, lanes ^ m]
    assert acc.dtype == F4
    return acc[:, 0]


def emulate(out, sel, target, loss_type="cosine", up=1.0, mutant=None):
    """The kernels' arithmetic in numpy, fp32 operation by operation in their order (module docstring) -> {"loss": float32,
    "grad": float32 [n, d]}.  mutant: one of MUTANTS, the same arithmetic with that one defect:
      a  ka scaled by (1 + 3e-6)                               b  ka without its `sqrtf(a2) > eps` test
      c  the norms not clamped in the gradient                 d  the target row (and its statistics) taken at the rank of r among
      e  the butterfly started at 16: lanes >= 32 lost            the selected rows instead of pos[r]
      f  the last partial 256-column step left out of the      g  the loss mean without the rows from 1024 * (n_sel // 1024) on
         statistics (d > 256)                                     (n_sel >= 1024)
      h  L1: +s for a == b"""
    assert mutant is None or mutant in MUTANTS
    n, d = out.shape
    n_sel = sel.shape[0]
    x, y = out[sel], target
    up = F4(up)
    grad = np.zeros((n, d), dtype=F4)
    in_mean = n_sel if not (mutant == "g" and n_sel >= 1024) else 1024 * (n_sel // 1024)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if loss_type == "l1":
            val = _wave_sums(np.abs(x - y), mutant)
            loss = F4(np.sum(val[:in_mean].astype(F8)) * (1.0 / (F8(n_sel) * F8(d))))
            s = up / (F4(n_sel) * F4(d))
            diff = x - y
            grad[sel] = np.where(diff > 0, s, np.where(diff < 0, -s, s if mutant == "h" else F4(0)))
            return {"loss": loss, "grad": grad}
        dot, a2, b2 = _wave_sums(x * y, mutant), _wave_sums(x * x, mutant), _wave_sums(y * y, mutant)
        na, nb = np.maximum(np.sqrt(a2), EPS32), np.maximum(np.sqrt(b2), EPS32)
        val = F4(1) - dot / (na * nb)
        loss = F4(np.sum(val[:in_mean].astype(F8)) * (1.0 / F8(n_sel)))
        if mutant == "d":                                                # row sel[j] pairs with the target at its rank in sorted(sel)
            rank = np.argsort(np.argsort(sel))
            y, dot, a2, b2 = y[rank], dot[rank], a2[rank], b2[rank]
            na, nb = na[rank], nb[rank]
        if mutant == "c":
            na, nb = np.sqrt(a2), np.sqrt(b2)
        s = -up / F4(n_sel)
        kb = s / (na * nb)
        ka = (-s * dot) / (((na * na) * na) * nb)
        if mutant != "b":
            ka = np.where(np.sqrt(a2) > EPS32, ka, F4(0))
        if mutant == "a":
            ka = ka * F4(1 + 3e-6)
        g = kb[:, None] * y + ka[:, None] * x
        assert g.dtype == F4 and kb.dtype == F4 and ka.dtype == F4 and val.dtype == F4
        grad[sel] = g
    return {"loss": loss, "grad": grad}


def dense_check(got, ref_loss, ref_grad, up=1.0):
    """Would the criteria of test_gpu_dense.py::test_distill_loss_forward_and_gradient pass `got`?  -> (gradient criterion: every
    row within 2e-6 of the row's largest element;  loss criterion: 1e-6 relative to max(1, |loss|))."""
    g = np.asarray(got["grad"], dtype=F8) / up
    scale = np.abs(ref_grad).max(axis=1, keepdims=True)
    return (bool((np.abs(g - ref_grad) <= 2e-6 * scale + 1e-30).all()),
            bool(abs(float(got["loss"]) - ref_loss) <= 1e-6 * max(1.0, abs(ref_loss))))


def dense_inputs(n, n_sel, d, loss_type="cosine"):
    """The inputs of test_gpu_dense.py's loss test at one of its shapes (same distribution: 2.5 randn rows, unit fp16 targets,
    a SORTED selection)."""
    g = np.random.default_rng(_seed("dense", n, n_sel, d))
    out = (2.5 * g.standard_normal((n, d))).astype(F4)
    sel = np.sort(g.permutation(n)[:n_sel]).astype(np.int64)
    return out, sel, _unit_fp16(g, n_sel, d)
