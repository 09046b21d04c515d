"""The arithmetic contract of the open-vocabulary query in one place (plain helper module; imported by test_query_bounds_cpu.py and
test_gpu_query_bounds.py).  Stated once more in the header of csrc/query.hip and beside osn_cosine_query in include/openscene_amd.h.

Scores.  xh = fp16_rne(x) is the reference's `.half()` (overflow becomes +-inf); S = sum_k xh_k t_k and A = sum_k |xh_k| |t_k|, both
in float64.  Rounding is monotone, so every fp16 score a kernel writes must satisfy

    fp16_rne(S - c A)  <=  got  <=  fp16_rne(S + c A),        c = conv_bounds.FWD_C = 2e-6

(the project's bound for an fp32-accumulating MFMA contraction), float64 rounded to fp16 in ONE step (numpy's astype(float16) from
float64).  Where S is +-inf or NaN both ends are S and the score must be that value.  test_query_bounds_cpu.py shows that an fp32
chain in ascending k meets this on every operand kind, and that six kinds of subtly wrong kernel do not.

Labels.  label = torch.max(scores.cpu(), 1)[1] of the kernel's OWN fp16 scores on every row (the first NaN wins, otherwise the lowest
column among equal maxima, -0.0 == +0.0); against float64 the label equals the float64 argmax wherever the winner's lower interval
end exceeds every other column's upper end (`decided`).

Operands.  Six kinds of feature rows (KINDS) against unit-norm fp16 text rows.  The first RESERVED = 4 channels belong to the planted
rows: ordinary rows are zero there, and the text carries fixed magnitudes and planted signs in them, so that the planted feature
rows 0 .. N_PLANTED-1 produce (for c >= 4; PLANTED names the rows)
    rows 0-5, 6-11, 12-13  x = 3000, -3000, NaN everywhere: tests/test_gpu_eval.py::features (text row 0 is 1/sqrt(d) everywhere:
                           its score overflows to +-inf from d = 520 on);
    inf_two                -inf in column 0, +inf in every other column: the first +inf, column 1, wins;
    nan_among              -inf, +inf, NaN in column 2, +inf ...: the NaN wins.  (A score kernel cannot make a NaN among FINITE
                           scores: a NaN needs an infinite xh, and inf * t is +-inf or NaN in every column.  ops.rows_argmax, which
                           is handed its scores, gets such rows: rows_argmax_scores.)
    all_neg_inf            every column -inf: label 0;
    signed_zeros           -0.0 in the even columns, +0.0 in the odd ones: label 0;
    zero                   an all-zero feature row: every score +0.0, label 0.
Text rows 3 and c-1 duplicate rows 1 and c // 2 (c > 4), at a QUARTER of the norm: exact ties then occur on the planted rows and on
a few ordinary ones, rarely enough for the 5 % cap on float64-undecided rows to hold at 33 labels (asserted on the CPU).

Ensemble (oracle/query.py: query_ensemble in float64).  The kernel's denominator ||x|| + 1e-5 is an fp32 sum in another order, so
fp16_rne(x / den) may differ by one fp16 step on rare elements.  That is carried as an interval: xh_lo = fp16_rne(q (1 - DELTA)),
xh_hi = fp16_rne(q (1 + DELTA)) with q the float64 quotient, S bounded term by term, widened by c A.  DELTA = 4.5e-6: the relative
error of fp32 sqrt(sum x^2) + 1e-5 followed by an fp32 divide against float64, measured in test_query_bounds_cpu.py over the rows
of ENSEMBLE_SHAPES with the sum of squares taken in two orders -- ascending (one sequential chain, whose rounding errors drift):
worst 3.1e-7 at d = 72, 7.8e-7 at d = 512, 1.07e-6 at d = 768; the kernel's lanes-then-butterfly order (norm_fp32): worst 2.0e-7 at
every d -- times four, rounded up.
"""
import collections
import functools

import numpy as np
import torch

import conv_bounds as cb

C = cb.FWD_C
DELTA = 4.5e-6
KINDS = ("unit", "row_scales", "wide_elements", "coherent", "cancellation", "half_ties")
RESERVED = 4                       # channels 0 .. 3: zero in ordinary rows
BIG = 1e5                          # inf as fp16
PLANTED = {"pos3000": slice(0, 6), "neg3000": slice(6, 12), "nan": slice(12, 14), "inf_two": 14, "nan_among": 15, "all_neg_inf": 16,
           "signed_zeros": 17, "zero": 18}
N_PLANTED = 19


def features(kind, n, d, g):
    """[n, d] fp32 ordinary rows of an operand kind."""
    x = torch.randn(n, d, generator=g)
    if kind == "unit":               # the inputs of tests/test_gpu_dense.py
        x = x / x.norm(dim=1, keepdim=True) * (0.5 + 1.5 * torch.rand(n, 1, generator=g))
    elif kind == "row_scales":       # per-row magnitudes 1e-5 .. 1e3
        x = x * (10.0 ** (torch.rand(n, 1, generator=g) * 8 - 5))
    elif kind == "wide_elements":    # per-element magnitudes over eight decades: many become fp16 subnormals or zero
        x = x * (10.0 ** (torch.rand(n, d, generator=g) * 8 - 6))
    elif kind == "coherent":         # all positive (the text too): fp32 accumulation error adds up
        x = x.abs() * 0.05
    elif kind == "cancellation":     # channel pairs (a, -a(1 + 2^-9)) against equal text entries: scores cancel to ~2^-9 of A
        x[:, 1::2] = -x[:, 0::2] * (1 + 2.0 ** -9)
    elif kind == "half_ties":        # fp16 rounding ties and near-ties: truncation instead of round-to-nearest-even shows in xh
        x = (x * 4).round() / 4 + 2.0 ** -12 * torch.randint(-1, 2, (n, d), generator=g)
    else:
        raise ValueError(kind)
    return x


def text(kind, c, d, g):
    """[c, d] fp16 unit-norm text rows that go with features(kind, ...), before planting."""
    t = torch.randn(c, d, generator=g)
    t = t / t.norm(dim=1, keepdim=True)
    if kind == "coherent":
        t = t.abs()
    elif kind == "cancellation":
        t[:, 1::2] = t[:, 0::2]
    return t


def plant(x, t):
    """The planted rows and text entries of the module docstring, in place; -> (x, t.half())."""
    n, d = x.shape
    c = t.shape[0]
    assert n >= N_PLANTED and d >= 2 * RESERVED
    t[0] = 1.0 / d ** 0.5
    if c > 4:
        t[1] *= 0.25
        t[c // 2] *= 0.25
        t[3] = t[1]
        t[c - 1] = t[c // 2]
    cols = torch.arange(c)
    sa = torch.where(cols == 0, -1.0, 1.0)
    sb = torch.where(cols == 2, -sa, sa)
    t[:, 0] = sa / 16
    t[:, 1] = sb / 16
    t[:, 2] = 1.0 / 16
    t[:, 3] = 0.01 * torch.where(cols % 2 == 0, -1.0, 1.0)
    x[:, :RESERVED] = 0.0
    x[PLANTED["pos3000"]] = 3000.0
    x[PLANTED["neg3000"]] = -3000.0
    x[PLANTED["nan"]] = float("nan")
    for name in ("inf_two", "nan_among", "all_neg_inf", "signed_zeros", "zero"):
        x[PLANTED[name]] = 0.0
    x[PLANTED["inf_two"], 0] = BIG
    x[PLANTED["nan_among"], 0] = BIG
    x[PLANTED["nan_among"], 1] = BIG
    x[PLANTED["all_neg_inf"], 2] = -BIG
    x[PLANTED["signed_zeros"], 3] = 1e-6          # an fp16 subnormal; times 0.01 it is below half the smallest one
    return x, t.half()


@functools.lru_cache(maxsize=6)
def operands(kind, n_rows, d, c):
    """(features fp32 [max(n_rows, N_PLANTED), d], text fp16 [c, d]); shared, never modified."""
    g = torch.Generator().manual_seed(cb._seed("query", kind, n_rows, d, c))
    n = max(n_rows, N_PLANTED)
    return plant(features(kind, n, d, g), text(kind, c, d, g))


def gather_index(n, n_rows, tag=0):
    """int64 [n] point -> feature row: every planted row, row 0 and the last row present, one neighbouring duplicate (random draws
    add more).  A single point reads the nan_among row."""
    if n == 1:
        return torch.tensor([PLANTED["nan_among"]])
    assert n >= N_PLANTED + 3
    g = torch.Generator().manual_seed(cb._seed("gather", n, n_rows, tag))
    idx = torch.randint(0, n_rows, (n,), generator=g)
    idx[:N_PLANTED] = torch.arange(N_PLANTED)
    idx[N_PLANTED + 1] = idx[N_PLANTED]
    idx[n - 1] = n_rows - 1
    return idx


# ------------------------------------------------------------------------------------------------------------ the score interval
def fp16_rne(a):
    """float64 -> fp16 in one rounding step (overflow: +-inf)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float16)


Ref = collections.namedtuple("Ref", "S A lo hi")          # float64 S, A; fp16 interval ends


def interval(xh, t, c=C):
    """The contract's interval for fp16-valued features xh [n, d] (any float array holding fp16 values) and text t [c, d]."""
    xh, t = np.asarray(xh, dtype=np.float64), np.asarray(t, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        S = xh @ t.T
        A = np.abs(xh) @ np.abs(t).T
        fin = np.isfinite(S)
        return Ref(S, A, fp16_rne(np.where(fin, S - c * A, S)), fp16_rne(np.where(fin, S + c * A, S)))


def interval_between(x_lo, x_hi, t, c=C):
    """The interval for features known only elementwise, x_lo <= xh <= x_hi (finite): S bounded term by term, widened by c A."""
    x_lo, x_hi, t = (np.asarray(a, dtype=np.float64) for a in (x_lo, x_hi, t))
    assert np.isfinite(x_lo).all() and np.isfinite(x_hi).all() and (x_lo <= x_hi).all()
    tp, tn = np.maximum(t, 0.0), np.minimum(t, 0.0)
    s_lo = x_lo @ tp.T + x_hi @ tn.T
    s_hi = x_hi @ tp.T + x_lo @ tn.T
    A = np.maximum(np.abs(x_lo), np.abs(x_hi)) @ np.abs(t).T
    return Ref(0.5 * (s_lo + s_hi), A, fp16_rne(s_lo - c * A), fp16_rne(s_hi + c * A))


def half(x):
    """The reference's .half() of an fp32 tensor, as float64 numpy."""
    return x.half().double().numpy()


@functools.lru_cache(maxsize=4)
def reference(kind, n_rows, d, c):
    """interval() of operands(kind, n_rows, d, c), per FEATURE row; computed once per (shape, kind), never modified."""
    x, t = operands(kind, n_rows, d, c)
    return interval(half(x), t.double().numpy())


def _as_np(scores):
    return scores.detach().cpu().numpy() if isinstance(scores, torch.Tensor) else np.asarray(scores)


def _wide(h):
    """fp16 values as float64 with +-inf at +-2^16, so that the midpoint towards 65504 is the overflow threshold 65520."""
    return np.clip(h.astype(np.float64), -65536.0, 65536.0)


def outside(got, ref, rows=None):
    """bool [n, c]: the scores that break the contract.  rows: the feature row of every score row (None: the identity)."""
    got = _as_np(got)
    assert got.dtype == np.float16
    lo, hi = (ref.lo, ref.hi) if rows is None else (ref.lo[rows], ref.hi[rows])
    assert got.shape == lo.shape, (got.shape, lo.shape)
    with np.errstate(invalid="ignore"):
        ok = ((lo <= got) & (got <= hi)) | (np.isnan(lo) & np.isnan(got))
    return ~ok


def worst_ratio(got, ref, rows=None, c=C):
    """(worst c' / c, number of scores outside): c' is the smallest constant that would take the score into its interval (0 where
    the score is the rounding of S itself; inf where a non-finite S is not met)."""
    got = _as_np(got)
    S, A = (ref.S, ref.A) if rows is None else (ref.S[rows], ref.A[rows])
    bad = outside(got, ref, rows)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        g = _wide(got)
        below = 0.5 * (g + _wide(np.nextafter(got, np.float16(-np.inf))))      # the rounding boundaries of the score
        above = 0.5 * (g + _wide(np.nextafter(got, np.float16(np.inf))))
        below = np.where(got == -np.inf, -np.inf, below)                        # (an infinite score has no boundary beyond it)
        above = np.where(got == np.inf, np.inf, above)
        need = np.maximum(np.maximum(below - S, S - above), 0.0) / A
        need = np.where(np.isfinite(S), np.where(A > 0, need, np.where(got == 0, 0.0, np.inf)), np.where(bad, np.inf, 0.0))
        need = np.where(np.isnan(need), np.inf, need)
    return (float(need.max()) / c if need.size else 0.0), int(bad.sum())


def within(got, ref, rows=None, label=""):
    ratio, n_bad = worst_ratio(got, ref, rows)
    print("%s: worst ratio %.3f, %d outside" % (label, ratio, n_bad))
    assert n_bad == 0, "%s: %d scores outside the interval, worst ratio %.2f" % (label, n_bad, ratio)
    return ratio


# ------------------------------------------------------------------------------------------------------------------- labels
def torch_max_labels(scores):
    """The label rule: torch.max on the CPU (the first NaN wins, otherwise the lowest column among equal maxima)."""
    s = scores.detach().cpu() if isinstance(scores, torch.Tensor) else torch.from_numpy(np.asarray(scores))
    return torch.max(s, 1)[1]


def rule_labels(scores, rule="torch_max"):
    """The label rule restated in numpy, and two wrong ones: "nan_never_wins" (v > best || v == best && col < besti from (-inf,
    none); an all-NaN row yields 0) and "raw_bits" (the maximum of monotone fp16 bit keys, -0 made +0, NaN left where its bits
    put it: above +inf when positive, below -inf when negative)."""
    s = _as_np(scores)
    n, c = s.shape
    if rule == "raw_bits":
        hb = s.astype(np.float16).view(np.uint16).astype(np.int64)
        hb = np.where(hb == 0x8000, 0, hb)
        ordk = np.where(hb & 0x8000, ~hb & 0xFFFF, hb | 0x8000)
        return torch.from_numpy(np.argmax((ordk << 16) | (0xFFFF - np.arange(c))[None, :], axis=1))
    v = s.astype(np.float64)
    nan = np.isnan(v)
    with np.errstate(invalid="ignore"):
        best = np.argmax(np.where(nan, -np.inf, v), axis=1)               # (argmax: the first of equal maxima; -0.0 == +0.0)
    if rule == "nan_never_wins":
        return torch.from_numpy(np.where(nan.all(1), 0, best))
    assert rule == "torch_max"
    return torch.from_numpy(np.where(nan.any(1), np.argmax(nan, axis=1), best))


def decided(ref):
    """(float64 argmax int64 [n], bool [n]: the winner's lower interval end exceeds every other column's upper end)."""
    lo, hi = ref.lo.astype(np.float64), ref.hi.astype(np.float64)
    n, c = lo.shape
    nan = np.isnan(ref.S).any(1)
    w = np.argmax(np.where(np.isnan(ref.S), -np.inf, ref.S), axis=1)
    if c == 1:
        return w, ~nan
    others = np.where(np.isnan(hi), np.inf, hi)
    others[np.arange(n), w] = -np.inf
    with np.errstate(invalid="ignore"):
        return w, ~nan & (lo[np.arange(n), w] > others.max(1))


def rows_argmax_scores(n, c, seed=0):
    """fp32 [n, c] scores for ops.rows_argmax (n >= 16): random with ties, and rows of NaN among finite scores (not in column 0; in
    two columns; in a column >= 64, which a lane reaches on its second trip), +inf in two columns, all -inf, signed zeros."""
    g = torch.Generator().manual_seed(cb._seed("rows_argmax", n, c, seed))
    s = torch.randn(n, c, generator=g)
    s[::5] = s[::5].round()
    last = c - 1
    s[1, min(1, last)] = float("nan")
    s[2, last] = float("nan")
    s[3, last] = float("nan")
    s[3, c // 2] = float("nan")
    s[4, min(2, last)] = float("inf")
    s[4, last] = float("inf")
    s[5] = float("-inf")
    s[6] = 0.0
    s[6, ::2] = -0.0
    s[7] = float("nan")
    s[8, 0] = float("inf")
    s[8, last] = float("nan")
    if c > 64:
        s[9, 64 + (c - 65) // 2] = float("nan")       # second trip, finite scores before and after
        s[10, 3] = float("inf")
        s[10, 70 % c] = float("nan")
        s[11, 64] = float("nan")
        s[11, 0] = float("nan")
    return s


# ------------------------------------------------------------------------------------------------------------------ ensemble
def norm_fp32(x, order):
    """fp32 sqrt(sum x^2) + 1e-5 of every row of an fp32 [n, d] array, the sum of squares taken in `order`: "ascending", or "lanes"
    = row_norm_kernel's (lane l adds the float4 at 4 l, 4 l + 256, ...: the four squares summed left to right, then added to the
    lane's sum; a butterfly over the 64 lanes, partner distance 32, 16, ... 1)."""
    x = np.asarray(x, dtype=np.float32)
    n, d = x.shape
    sq = x * x
    if order == "ascending":
        s = np.zeros(n, dtype=np.float32)
        for k in range(d):
            s = s + sq[:, k]
    else:
        assert order == "lanes" and d % 4 == 0
        lanes = np.zeros((n, 64), dtype=np.float32)
        for j0 in range(0, d, 256):
            for l in range(64):
                j = j0 + 4 * l
                if j < d:
                    lanes[:, l] = lanes[:, l] + (((sq[:, j] + sq[:, j + 1]) + sq[:, j + 2]) + sq[:, j + 3])
        m = 32
        while m >= 1:
            lanes = lanes + lanes[:, np.arange(64) ^ m]
            m >>= 1
        s = lanes[:, 0]
    return np.sqrt(s).astype(np.float32) + np.float32(1e-5)


def quotient_error(x, order):
    """Worst relative error of fp32 x / norm_fp32(x, order) against the float64 quotient x / (||x|| + 1e-5), over the non-zero
    elements whose quotient is a normal fp32."""
    x = np.asarray(x, dtype=np.float32)
    q32 = (x / norm_fp32(x, order)[:, None]).astype(np.float64)
    x64 = x.astype(np.float64)
    q64 = x64 / (np.sqrt((x64 * x64).sum(1)) + 1e-5)[:, None]
    m = np.abs(q64) > 1e-30
    return float((np.abs(q32 - q64)[m] / np.abs(q64)[m]).max())


def normalised_interval(x, t):
    """interval_between for the ensemble's normalised fp16 features of fp32 rows x (finite): q = x / (||x|| + 1e-5) in float64,
    xh in [fp16_rne(q (1 - DELTA)), fp16_rne(q (1 + DELTA))]."""
    x64 = np.asarray(x, dtype=np.float64)
    q = x64 / (np.sqrt((x64 * x64).sum(1)) + 1e-5)[:, None]
    a, b = fp16_rne(q * (1 - DELTA)).astype(np.float64), fp16_rne(q * (1 + DELTA)).astype(np.float64)
    return interval_between(np.minimum(a, b), np.maximum(a, b), t)


Ensemble = collections.namedtuple("Ensemble", "xd xf text gd gf sel decided ref_d ref_f")
# (points, voxels, d, c): query_kernel with one and with two column groups; query_wide_kernel at both widths, ragged last tile
ENSEMBLE_SHAPES = [(300, 200, 72, 33), (300, 200, 768, 161), (4129, 2000, 768, 160), (4129, 2000, 512, 65)]


@functools.lru_cache(maxsize=3)
def ensemble_case(n, n_vox, d, c):
    """The ensemble's operands and float64 reference (oracle/query.py: query_ensemble, restated in float64 numpy with one-step fp16
    roundings).  xd [n_vox, d] distilled and xf [n_vox, d] fusion features; point p reads xd[gd[p]] and xf[gf[p]], gf = a
    permutation of gd, so the `X1` / `g1` offsets differ from the `X0` / `g0` ones.  The fusion feature of a voxel is correlated
    with its distilled one (tests/test_gpu_dense.py: test_fused_head_ensemble_query_...), so that both sources win.  Voxel 0 is
    all zero in both sources: den = 1e-5, scores 0, label 0, distilled source kept.
    sel = the reference's pd.max < pf.max per point; decided = the intervals of the two maxima are disjoint; ref_d / ref_f = the
    score interval of each source's UN-normalised features per point."""
    g = torch.Generator().manual_seed(cb._seed("ensemble", n, n_vox, d, c))
    xd = torch.randn(n_vox, d, generator=g) * (0.5 + torch.rand(n_vox, 1, generator=g))
    corr = (xd * (0.6 + 0.8 * torch.rand(n_vox, 1, generator=g)) + 0.9 * xd.std() * torch.randn(n_vox, d, generator=g)).half().float()
    xd[0] = 0.0
    corr[0] = 0.0
    perm = torch.cat([torch.zeros(1, dtype=torch.int64), 1 + torch.randperm(n_vox - 1, generator=g)])     # (voxel 0 stays row 0)
    xf = torch.empty_like(corr)
    xf[perm] = corr
    t = torch.randn(c, d, generator=g)
    t = (t / t.norm(dim=1, keepdim=True)).half()
    gd = torch.randint(0, n_vox, (n,), generator=g)
    gd[0], gd[1], gd[2], gd[n - 1] = 0, 5, 5, n_vox - 1
    gf = perm[gd]
    tn = t.double().numpy()
    fd, ff = xd[gd].numpy(), xf[gf].numpy()
    nd, nf = normalised_interval(fd, tn), normalised_interval(ff, tn)

    def exact_max(f):
        f64 = f.astype(np.float64)
        q = f64 / (np.sqrt((f64 * f64).sum(1)) + 1e-5)[:, None]
        r = interval(fp16_rne(q), tn)
        return fp16_rne(r.S).astype(np.float64).max(1)

    sel = exact_max(fd) < exact_max(ff)
    lo_d, hi_d = nd.lo.astype(np.float64).max(1), nd.hi.astype(np.float64).max(1)
    lo_f, hi_f = nf.lo.astype(np.float64).max(1), nf.hi.astype(np.float64).max(1)
    dec = (hi_d < lo_f) | (lo_d > hi_f)
    return Ensemble(xd, xf, t, gd, gf, sel, dec, interval(half(xd[gd]), tn), interval(half(xf[gf]), tn))


def ensemble_scores_outside(scores, sel_got, ens):
    """bool [n, c]: the scores that break the contract of the source the kernel says it selected."""
    sel_got = _as_np(sel_got).astype(bool)
    return np.where(sel_got[:, None], outside(scores, ens.ref_f), outside(scores, ens.ref_d))
