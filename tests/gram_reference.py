"""What the PCA tests compare against (openscene_amd.pca, csrc/gram.hip), restated independently of the library:

    gram_f64        the Gram matrix and the column sums in float64 on the stored values with UNROUNDED normalised rows, with
                    the per-element abs-sums  sum |x_a x_b|  and  sum |x_a|
    operands        the fp16 operands h of the contract, as float64 [L, d] (what the constant is measured against)
    bank_gram, bank_gram_fp8
                    CPU stand-ins for the two kernels' ops: operands rounded to fp16, products in float32 (exact), a group
                    cut into slices of SLICE entries, a slice added entry by entry -- the longest chain a slice allows --
                    a group's partials added in slice order, the triangle mirrored (tests/test_pca_cpu.py)
    worst_ratio     the abs-sum bound of tests/pool_reference.py, restated
    bound_case      the inputs the bound is measured on (CPU, stand-in) and held on (GPU, kernel): the same arrays
    planted         three scenes of three orthogonal feature classes, for the principal directions and the end-to-end test

The operand of an entry with stored row v:  h = fp16(v / (||v|| + 1e-5))  (run/evaluate.py:305,310) or  h = fp16(v)."""
import functools

import torch

import search_fp8_reference as f8

SLICE = 2048                     # == ops.BANK_GRAM_SLICE == OSN_BANK_GRAM_SLICE (tests/test_pca_cpu.py asserts it)

# The bound of a Gram element:  |gram - gram_f64| <= (R + GRAM_C) * abs-gram + 6e-8 |want| + 1e-37, and of a sum the same with
# R_SUM and abs-sum.  R = 2^-10 + 2^-20 covers (1 + 2^-11)^2 - 1: the two operands, each rounded once to fp16; R_SUM = 2^-11: one.  Both are 0 where
# the operands are exact (normalize = 0 on rows that fp16 holds).
# The rounding is RELATIVE only in fp16's normal range: a normalised component below 2^-14 rounds with an absolute error of up
# to 2^-25, which R does not cover in a group of one row.  The rows of the bound cases therefore keep every component of the
# unit direction at 2^-12 or above in magnitude (_directions): after the normalisation, the fp16 storage and the e4m3 storage
# (a relative 2^-4) the components stay above 2^-13.  Smaller components are held to the bound plus the absolute terms of the
# rounding (tiny_case, tiny_slack below), and are the exact tests' ground (integers, one row).
# GRAM_MEASURED_RATIO is the worst error / abs-sum of the stand-in below against the float64 evaluation on the SAME rounded
# operands, over every bound_case, Gram elements and sums (tests/test_pca_cpu.py measures it again and holds the constant to
# it).  The stand-in adds a slice's 2048 terms one after the other -- the longest chain a slice allows; the kernel adds 32
# products inside an MFMA and chains 64 of those.  GRAM_C = 4 x measured: one factor of 2 for the different order inside a
# slice, one for the fused accumulation of the matrix pipe and the fp32 scale of the normalisation.  It must stay at or below
# 2e-5, the loosest abs-sum constant the project accepts for a long fp32 contraction.
R_GRAM = 2.0 ** -10 + 2.0 ** -20
R_SUM = 2.0 ** -11
# The record is the measurement rounded up in its third digit (4.319e-6 at fp8-528-plain: a group of 2049 unit rows; the
# float32 norm of the stand-in is rounded once from a float64 sum, and a rank-one float32 update rounds once per element
# whether fused or not: the same bits on every IEEE host).
GRAM_MEASURED_RATIO = 4.32e-6
GRAM_C = 4 * GRAM_MEASURED_RATIO
GRAM_C_CAP = 2e-5


# ------------------------------------------------------------------------------------------------------ float64
def _entries(starts, rows, n_entries):
    starts = starts.cpu().long()
    g = starts.shape[0] - 1
    length = starts[1:] - starts[:-1]
    group = torch.repeat_interleave(torch.arange(g), length)
    rows = torch.arange(n_entries) if rows is None else rows.cpu().long()
    return g, group, rows


def _moments_f64(x, starts):
    """x float64 [L, d], entries in group order -> (gram, abs-gram [G, d, d], sum, abs-sum [G, d])"""
    starts = starts.cpu().long().tolist()
    g, d = len(starts) - 1, x.shape[1]
    gram, bound = torch.zeros(g, d, d, dtype=torch.float64), torch.zeros(g, d, d, dtype=torch.float64)
    total, tbound = torch.zeros(g, d, dtype=torch.float64), torch.zeros(g, d, dtype=torch.float64)
    for i in range(g):
        xi = x[starts[i]:starts[i + 1]]
        if xi.shape[0]:
            ai = xi.abs()
            gram[i], bound[i], total[i], tbound[i] = xi.t() @ xi, ai.t() @ ai, xi.sum(0), ai.sum(0)
    return gram, bound, total, tbound


def gram_f64(values, starts, rows, normalize):
    """values [N, d] (the stored values: features.float() or dequantize()); starts int64 [G + 1]; rows int64 [L] or None.
    -> (gram [G, d, d], abs_gram, sum [G, d], abs_sum, count [G]), float64 / int64 on the CPU, the rows NOT rounded."""
    v = values.detach().cpu().double()
    n_entries = int(starts[-1])
    g, group, rows = _entries(starts, rows, n_entries)
    x = v[rows]
    if normalize:
        x = x / (x.norm(dim=-1, keepdim=True) + 1e-5)
    return _moments_f64(x, starts) + (torch.bincount(group, minlength=g),)


def worst_ratio(got, want, bound, c):
    """(worst err / lim, elements beyond lim): lim = c * abs-sum + half an ulp of the fp32 result + a floor at the denormal edge."""
    want = want.detach().double().cpu()
    err = (got.detach().double().cpu() - want).abs()
    lim = c * bound + 6e-8 * want.abs() + 1e-37
    bad = ~(err <= lim)                                       # (a NaN is beyond every bound)
    return (float(torch.nan_to_num(err / lim, nan=float("inf")).max()) if err.numel() else 0.0), int(bad.sum())


def error_over_abs_sum(got, want, bound):
    """The worst |got - want| / abs-sum over the elements with a non-zero abs-sum (what GRAM_MEASURED_RATIO records)."""
    err = (got.detach().double().cpu() - want).abs()
    some = bound > 0
    return float((err[some] / bound[some]).max()) if bool(some.any()) else 0.0


# ------------------------------------------------------------------------------------------------------ stand-ins
def _operands_f16(c, scale, rows, normalize):
    """c float32 [N, d]: the fp16 rows widened, or the code values; scale float32 [N] = 2^e.  -> h fp16 [L, d] of the rows `rows`"""
    x, sc = c[rows], scale[rows]
    # (the sum of squares in float64, rounded once: the same float32 on every host, whatever the order of its reduction)
    s = sc / (x.double().square().sum(dim=1).float().sqrt() * sc + 1e-5) if normalize else sc
    return (x * s[:, None]).half()


def _gram_f32(c, scale, starts, rows, normalize, n_entries, err):
    n, d = c.shape
    g, group, rows = _entries(starts, rows, n_entries)
    bad = (rows < 0) | (rows >= n)
    if err is not None and bool(bad.any()):
        err |= 8
    ok = ~bad
    safe = torch.where(ok, rows, torch.zeros_like(rows))
    h = _operands_f16(c, scale, safe, normalize).float() if n else torch.zeros(n_entries, d)
    h[bad] = 0                                                # (a skipped entry adds nothing; +0 leaves every bit)
    starts = starts.cpu().long()
    length = starts[1:] - starts[:-1]
    n_slices = (length + SLICE - 1) // SLICE
    base = torch.zeros(g + 1, dtype=torch.int64)
    base[1:] = torch.cumsum(n_slices, 0)
    slice_group = torch.repeat_interleave(torch.arange(g), n_slices)
    slice_k = torch.arange(int(base[-1])) - base[slice_group]
    e0 = starts[slice_group] + slice_k * SLICE
    e1 = torch.minimum(e0 + SLICE, starts[slice_group + 1])
    pgram = torch.zeros(int(base[-1]), d, d, dtype=torch.float32)
    psum = torch.zeros(int(base[-1]), d, dtype=torch.float32)
    pc = torch.zeros(int(base[-1]), dtype=torch.int64)
    for j in range(SLICE):                                   # entry j of every slice: a slice is added entry by entry
        live = torch.nonzero(e0 + j < e1).reshape(-1)
        if live.numel() == 0:
            break
        i = e0[live] + j
        # h_a * h_b is exact in float32 (two 11-bit significands), so the rank-one update rounds once per element, fused or not
        pgram[live] = torch.baddbmm(pgram[live], h[i][:, :, None], h[i][:, None, :])
        psum[live] = psum[live] + h[i]
        pc[live] = pc[live] + ok[i].long()
    gram = torch.zeros(g, d, d, dtype=torch.float32)
    total = torch.zeros(g, d, dtype=torch.float32)
    count = torch.zeros(g, dtype=torch.int64)
    for k in range(int(n_slices.max()) if g else 0):         # a group's partials in slice order
        live = torch.nonzero(n_slices > k).reshape(-1)
        gram[live] = gram[live] + pgram[base[live] + k]
        total[live] = total[live] + psum[base[live] + k]
        count[live] = count[live] + pc[base[live] + k]
    upper = torch.triu(gram)                                  # the triangle on and above the diagonal, mirrored
    return upper + torch.triu(gram, 1).transpose(1, 2), total, count


def _code_rows(codes, exps):
    return f8.code_values().float()[codes.long()], torch.ldexp(torch.ones(exps.shape[0]), exps.int())


def bank_gram(bank, starts, rows=None, normalize=True, n_entries=None, err=None):
    n_entries = rows.shape[0] if rows is not None else int(n_entries)
    return _gram_f32(bank.float(), torch.ones(bank.shape[0]), starts, rows, normalize, n_entries, err)


def bank_gram_fp8(codes, exps, starts, rows=None, normalize=True, n_entries=None, err=None):
    n_entries = rows.shape[0] if rows is not None else int(n_entries)
    c, sc = _code_rows(codes, exps)
    return _gram_f32(c, sc, starts, rows, normalize, n_entries, err)


def operands(kind, stored, starts, rows, normalize):
    """The contract's fp16 operands of every entry as float64 [L, d]; `stored` = the fp16 rows, or (codes, exps)."""
    c, sc = (stored.float(), torch.ones(stored.shape[0])) if kind == "fp16" else _code_rows(*stored)
    _, _, rows = _entries(starts, rows, int(starts[-1]))
    return _operands_f16(c, sc, rows, normalize).double()


def rounded_moments_f64(kind, stored, starts, rows, normalize):
    """(gram, abs-gram, sum, abs-sum) in float64 on the rounded operands: what only the accumulation separates the stand-in from."""
    return _moments_f64(operands(kind, stored, starts, rows, normalize), starts)


# ------------------------------------------------------------------------------------------------------ bound cases
S = SLICE
FULL = (0, 1, S - 1, S, S + 1, 2 * S + 3)                    # every length around a slice edge: with the small dims
CROSS = (0, 1, 40, S + 1)                                    # one group across a slice edge
SHORT = (0, 1, 40, 300)
# (rows scaled over six decades, normalize)
VARIANTS = {"plain": (False, True), "scaled": (True, True), "raw": (True, False)}
# one tile | five tiles, the last of 8 / 16 columns | six whole tiles | eight: BANK_POOL_MAX_DIM
DIMS = {"fp16": (16, 24, 520, 768, 1024), "fp8": (16, 528, 768, 1024)}
FLOOR = 2.0 ** -12


def _lengths(kind, d, variant):
    if d <= 24:
        return FULL
    if d < 768:
        return CROSS
    return CROSS if (kind, d, variant) == ("fp16", 768, "plain") else SHORT      # the one case of d >= 768 across a slice edge


def _directions(n, d, gen):
    """Unit rows whose every component is at least FLOOR in magnitude (see the note on R above)."""
    x = torch.nn.functional.normalize(torch.randn(n, d, generator=gen), dim=1)
    x = torch.where(x.abs() < FLOOR, torch.where(x < 0, -FLOOR, FLOOR).to(x.dtype), x)
    return torch.nn.functional.normalize(x, dim=1)


def _rows_fp16(n, d, gen, scaled):
    x = _directions(n, d, gen)
    if scaled:                                               # the largest magnitude of a row from 0.02 to 2e4: every value of
        x = x / x.abs().amax(dim=1, keepdim=True) * 0.02 * torch.pow(10.0, 6 * torch.rand(n, 1, generator=gen))
    else:                                                    # the row, and of its e4m3 image (exponent -14 .. 6), is an fp16 value
        x = x * (0.5 + 1.5 * torch.rand(n, 1, generator=gen))
    return x.half()


def _csr(lengths):
    starts = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    starts[1:] = torch.cumsum(torch.tensor(lengths, dtype=torch.int64), 0)
    return starts


def case_names():
    names = ["%s-%d-%s" % (kind, d, v) for kind in ("fp16", "fp8") for d in DIMS[kind] for v in VARIANTS]
    for kind, d in (("fp16", 24), ("fp8", 16)):
        names += ["%s-%d-%s" % (kind, d, s) for s in ("many", "none", "scenes")]
    return names


@functools.lru_cache(maxsize=None)
def bound_case(name):
    """-> dict(kind, scenes (fp16 row matrices, one per scene of the bank), starts, rows or None, normalize)."""
    kind, d, variant = name.split("-")
    d = int(d)
    gen = torch.Generator().manual_seed(sum(ord(ch) for ch in name))
    if variant in VARIANTS:
        scaled, normalize = VARIANTS[variant]
        lengths, n = list(_lengths(kind, d, variant)), 700
    elif variant == "many":                                  # 300 groups, more than half of them empty, duplicates
        scaled, normalize = False, True
        lengths = [0] * 300
        for g in torch.randperm(300, generator=gen)[:120].tolist():
            lengths[g] = int(torch.randint(1, 40, (1,), generator=gen))
        lengths[7], lengths[299], n = S + 9, 2 * S, 500
    elif variant == "none":                                  # no entry at all
        scaled, normalize, lengths, n = False, True, [0, 0, 0], 40
    else:                                                    # scene ranges: no index array, the middle scene empty
        sizes = [S + 5, 0, 40]
        return {"kind": kind, "scenes": [_rows_fp16(m, d, gen, False) for m in sizes], "starts": _csr(sizes), "rows": None,
                "normalize": True}
    total = sum(lengths)
    return {"kind": kind, "scenes": [_rows_fp16(n, d, gen, scaled)], "starts": _csr(lengths),
            "rows": torch.randint(0, n, (total,), generator=gen), "normalize": normalize}


# ---- components below fp16's normal range: the one ground the bound cases leave out, held to the bound with its absolute terms
TINY_LENGTHS = (1,) * 40 + (2, 5, 40, 300)            # forty groups of one row: where the relative term alone fails
TINY_DIM = 768


@functools.lru_cache(maxsize=None)
def tiny_case(kind):
    """Rows as `search_reference.unit_rows` draws them, times 10^-3 .. 10^3 -- NO floor: about one normalised component in 700 lies
    below 2^-14 -- in groups from one row up.  -> a bound_case dict, normalize = True"""
    gen = torch.Generator().manual_seed(768 + len(kind))
    x = torch.nn.functional.normalize(torch.randn(700, TINY_DIM, generator=gen), dim=1)
    x = (x * torch.pow(10.0, 6 * torch.rand(700, 1, generator=gen) - 3)).half()
    total = sum(TINY_LENGTHS)
    return {"kind": kind, "scenes": [x], "starts": _csr(TINY_LENGTHS), "rows": torch.randint(0, 700, (total,), generator=gen),
            "normalize": True}


def tiny_slack(abs_sum, count):
    """What a rounding to fp16 adds where it is absolute: an operand is within 2^-11 |x| + 2^-25 of x whatever its size, so
    |h_a h_b - x_a x_b| <= R |x_a x_b| + 2^-25 (1 + 2^-11) (|x_a| + |x_b|) + 2^-50 per entry.
    abs_sum [G, d] = sum |x_a|, count [G] -> (to add to a Gram element's limit [G, d, d], to a sum's limit [G, d])"""
    n = count.double()
    gram = 2.0 ** -25 * (1 + 2.0 ** -11) * (abs_sum[:, :, None] + abs_sum[:, None, :]) + 2.0 ** -50 * n[:, None, None]
    return gram, 2.0 ** -25 * n[:, None].expand_as(abs_sum)


def beyond(got, want, bound, c, slack):
    """(worst err / lim, elements beyond lim) with lim = worst_ratio's + slack"""
    want = want.detach().double().cpu()
    err = (got.detach().double().cpu() - want).abs()
    lim = c * bound + 6e-8 * want.abs() + 1e-37 + slack
    return float(torch.nan_to_num(err / lim, nan=float("inf")).max()), int((~(err <= lim)).sum())


def case_r(case, stored_values):
    """(R of the Gram elements, R of the sums) of a case: 0 where the operands are exact -- not normalised, and every stored value
    an fp16 value (checked here, not assumed)."""
    if case["normalize"]:
        return R_GRAM, R_SUM
    v = stored_values.detach().cpu().double()
    assert torch.equal(v.half().double(), v), "a raw case must hold fp16 values only"
    return 0.0, 0.0


# ------------------------------------------------------------------------------------------------------ planted scenes
PLANT_DIM = 64
PLANT_SHARES = ((5, 2, 1), (2, 4, 2), (1, 2, 5))             # clusters of class 0, 1, 2 per scene (8 clusters each)
PLANT_POINTS = 250                                           # per cluster
PLANT_NOISE = 0.02                                           # per component: 0.16 in norm over 64 components, beside unit classes
# The colours of the planted bank (one basis for the whole bank, quantiles 0.01 / 0.99), measured on the float64 reference --
# float64 rows, float64 eigenvectors, the float64 quantile map -- on the stored values of the fp16 and of the fp8 bank: the class
# mean colours are 248.5 (fp16) and 249.5 (fp8) levels apart at least, the RMS distance of a class's colours to their mean is
# 54.2 (fp16) and 55.6 (fp8) at most (the third channel is noise).  A margin of two either way on the worse of each:
PLANT_BETWEEN_MIN = 124.0
PLANT_SPREAD_MAX = 112.0


@functools.lru_cache(maxsize=None)
def planted(seed=23):
    """Three scenes of 8 clusters x 250 points: a cluster fills a cube of 0.4 m, the cubes stand a metre apart; a point's
    feature is its cluster's class direction (three orthonormal directions) plus Gaussian noise, times a scale in 0.5 .. 2.
    -> dict(feats [fp16 per scene], xyz [float32 per scene], dirs float32 [3, d], cls [int64 per scene, per point],
            plane float64 [2, d]: an orthonormal basis of the plane of the class differences)"""
    gen = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(PLANT_DIM, 3, generator=gen))
    dirs = q.t().contiguous()
    feats, xyz, cls = [], [], []
    for shares in PLANT_SHARES:
        of_cluster = torch.repeat_interleave(torch.arange(3), torch.tensor(shares))[torch.randperm(8, generator=gen)]
        f, p, m = [], [], []
        for c in range(8):
            corner = torch.tensor([float(c % 4), float(c // 4), 0.0]) + 0.05
            p.append(corner + 0.4 * torch.rand(PLANT_POINTS, 3, generator=gen))
            scale = 0.5 + 1.5 * torch.rand(PLANT_POINTS, 1, generator=gen)
            f.append(scale * (dirs[of_cluster[c]] + PLANT_NOISE * torch.randn(PLANT_POINTS, PLANT_DIM, generator=gen)))
            m.append(torch.full((PLANT_POINTS,), int(of_cluster[c])))
        shuffle = torch.randperm(8 * PLANT_POINTS, generator=gen)
        feats.append(torch.cat(f)[shuffle].half())
        xyz.append(torch.cat(p)[shuffle].float())
        cls.append(torch.cat(m)[shuffle])
    diff = torch.stack([dirs[0] - dirs[1], dirs[0] - dirs[2]]).double()
    plane = torch.linalg.qr(diff.t())[0].t().contiguous()
    return {"feats": feats, "xyz": xyz, "dirs": dirs, "cls": cls, "plane": plane}


def plane_alignment(components, plane):
    """The smallest singular value of (the first two components) x plane^T: 1 when they span the plane."""
    return float(torch.linalg.svdvals(components[:2].double() @ plane.double().t()).min())


def sign_rule_holds(components):
    """Every component's entry of largest magnitude (the lowest index among equals) is positive."""
    c = components.reshape(-1, components.shape[-1])
    top = c.abs().argmax(dim=-1, keepdim=True)
    return bool((torch.gather(c, -1, top) > 0).all())


def colors_f64(coords, lo=0.01, hi=0.99):
    """uint8 [N, 3] of float64 coordinates [N, >= 3]: the quantile map restated."""
    x = coords[:, :3].double()
    n = x.shape[0]
    ranked = torch.sort(x, dim=0)[0]
    a, b = ranked[int(round(lo * (n - 1)))], ranked[int(round(hi * (n - 1)))]
    out = torch.full_like(x, 128.0)
    for j in range(3):
        if b[j] > a[j]:
            out[:, j] = torch.round(((x[:, j] - a[j]) / (b[j] - a[j])).clamp(0, 1) * 255)
    return out.to(torch.uint8)


def class_colour_stats(rgb, cls):
    """(the smallest distance between two class mean colours, the largest within-class RMS distance to the class mean)"""
    rgb = rgb.double().cpu()
    means = torch.stack([rgb[cls == c].mean(0) for c in range(3)])
    spread = max(float((rgb[cls == c] - means[c]).norm(dim=1).square().mean().sqrt()) for c in range(3))
    between = min(float((means[i] - means[j]).norm()) for i in range(3) for j in range(i + 1, 3))
    return between, spread
