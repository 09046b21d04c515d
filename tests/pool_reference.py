"""What the pool tests compare against (openscene_amd.descriptors, csrc/pool.hip), restated independently of the library:

    pool_f64        the descriptor sums in float64 on the stored values, with the per-element abs-sum  sum |term|
    bank_pool, bank_pool_fp8
                    CPU stand-ins for the two kernels' ops: float32, a group cut into chunks of BANK_POOL_CHUNK entries,
                    a chunk added entry by entry, a group's partials added in chunk order (tests/test_pool_cpu.py)
    objects_csr     PointGroups.from_objects restated with plain loops over point_object
    worst_ratio     the abs-sum bound of tests/conv_bounds.py, restated
    bound_case      the inputs the bound is measured on (CPU, stand-in) and held on (GPU, kernel): the same arrays
    planted         three scenes of spatial clusters of two feature classes, for the end-to-end test

The term of an entry with stored row v and weight w:  w * v / (||v|| + 1e-5)  (run/evaluate.py:305) or  w * v."""
import functools

import torch

import search_fp8_reference as f8
from search_reference import unit_rows

CHUNK = 512                      # == ops.BANK_POOL_CHUNK (tests/test_pool_cpu.py asserts it)

# The bound of the kernel's sums:  |sum - pool_f64| <= POOL_C * abs-sum + 6e-8 |want| + 1e-37  per element.
# POOL_MEASURED_RATIO is the worst error / abs-sum of the float32 stand-in below against pool_f64 over every bound_case
# (tests/test_pool_cpu.py::test_the_bound_constant_is_four_times_the_stand_ins_worst_ratio measures it again and holds the
# constant to it).  The stand-in adds a chunk's 512 terms one after the other -- the longest chain a chunk allows; the kernel
# deals a chunk to four waves (chains of 128) and adds the four.  POOL_C = 4 x measured: one factor of 2 for the different
# order inside a chunk (lanes and waves), one for fused multiply-adds and the fp32 norm.  It must stay at or below 2e-5,
# the loosest abs-sum constant the project accepts for a long fp32 contraction (WGRAD_C).
# The record is the measurement rounded up in its third digit (6.424e-7 at fp16-768-raw: rows scaled over six decades,
# weighted, not normalised -- elementwise float32 products added one by one, the same bits on every IEEE host; the normalised
# cases, whose float32 norm is a torch reduction whose order depends on the host, stay below 2.8e-7).
POOL_MEASURED_RATIO = 6.43e-7
POOL_C = 4 * POOL_MEASURED_RATIO
POOL_C_CAP = 2e-5


# ------------------------------------------------------------------------------------------------------ float64
def _entries(starts, rows, n_entries):
    starts = starts.cpu().long()
    g = starts.shape[0] - 1
    length = starts[1:] - starts[:-1]
    group = torch.repeat_interleave(torch.arange(g), length)
    rows = torch.arange(n_entries) if rows is None else rows.cpu().long()
    return g, group, rows


def pool_f64(values, starts, rows, weights, normalize):
    """values [N, d] (the stored values: features.float() or dequantize()); starts int64 [G + 1]; rows int64 [L] or None;
    weights [L] or None.  -> (sum [G, d], abs-sum [G, d], wsum [G], count [G]), float64 / int64 on the CPU."""
    v = values.detach().cpu().double()
    n_entries = int(starts[-1])
    g, group, rows = _entries(starts, rows, n_entries)
    w = torch.ones(n_entries, dtype=torch.float64) if weights is None else weights.detach().cpu().double()
    x = v[rows]
    if normalize:
        x = x / (x.norm(dim=-1, keepdim=True) + 1e-5)
    term = w[:, None] * x
    total = torch.zeros(g, v.shape[1], dtype=torch.float64).index_add_(0, group, term)
    bound = torch.zeros(g, v.shape[1], dtype=torch.float64).index_add_(0, group, term.abs())
    wsum = torch.zeros(g, dtype=torch.float64).index_add_(0, group, w)
    return total, bound, wsum, torch.bincount(group, minlength=g)


def worst_ratio(got, want, bound, c):
    """(worst err / lim, elements beyond lim): lim = c * abs-sum + half an ulp of the fp32 result + a floor at the denormal edge."""
    want = want.detach().double().cpu()
    err = (got.detach().double().cpu() - want).abs()
    lim = c * bound + 6e-8 * want.abs() + 1e-37
    bad = ~(err <= lim)                                       # (a NaN is beyond every bound)
    return (float(torch.nan_to_num(err / lim, nan=float("inf")).max()) if err.numel() else 0.0), int(bad.sum())


def error_over_abs_sum(got, want, bound):
    """The worst |got - want| / abs-sum over the elements with a non-zero abs-sum (what POOL_MEASURED_RATIO records)."""
    err = (got.detach().double().cpu() - want).abs()
    some = bound > 0
    return float((err[some] / bound[some]).max()) if bool(some.any()) else 0.0


# ------------------------------------------------------------------------------------------------------ stand-ins
def _pool_f32(c, scale, starts, rows, weights, normalize, n_entries, err):
    """c float32 [N, d]: the fp16 rows widened, or the code values; scale float32 [N] = 2^e (ones for fp16 rows)."""
    n, d = c.shape
    g, group, rows = _entries(starts, rows, n_entries)
    w = torch.ones(n_entries, dtype=torch.float32) if weights is None else weights.detach().cpu().float()
    bad_r = (rows < 0) | (rows >= n)
    bad_w = ~((w >= 0) & torch.isfinite(w))
    if err is not None:
        if bool(bad_r.any()):
            err |= 8
        if bool(bad_w.any()):
            err |= 16
    ok = ~(bad_r | bad_w)
    safe = torch.where(ok, rows, torch.zeros_like(rows))
    x, sc = (c[safe], scale[safe]) if n else (torch.zeros(n_entries, d), torch.ones(n_entries))
    s = w * sc
    if normalize:
        s = s / (x.square().sum(dim=1).sqrt() * sc + 1e-5)
    term = s[:, None] * x                                    # float32
    term[~ok] = 0                                            # (a skipped entry adds nothing; +0 leaves every bit)
    starts = starts.cpu().long()
    length = starts[1:] - starts[:-1]
    n_chunks = (length + CHUNK - 1) // CHUNK
    base = torch.zeros(g + 1, dtype=torch.int64)
    base[1:] = torch.cumsum(n_chunks, 0)
    chunk_group = torch.repeat_interleave(torch.arange(g), n_chunks)
    chunk_k = torch.arange(int(base[-1])) - base[chunk_group]
    e0 = starts[chunk_group] + chunk_k * CHUNK
    e1 = torch.minimum(e0 + CHUNK, starts[chunk_group + 1])
    psum = torch.zeros(int(base[-1]), d, dtype=torch.float32)
    pw = torch.zeros(int(base[-1]), dtype=torch.float32)
    pc = torch.zeros(int(base[-1]), dtype=torch.int64)
    wv = torch.where(ok, w, torch.zeros_like(w))
    for j in range(CHUNK):                                   # entry j of every chunk: a chunk is added entry by entry
        live = torch.nonzero(e0 + j < e1).reshape(-1)
        if live.numel() == 0:
            break
        i = e0[live] + j
        psum[live] = psum[live] + term[i]
        pw[live] = pw[live] + wv[i]
        pc[live] = pc[live] + ok[i].long()
    total = torch.zeros(g, d, dtype=torch.float32)
    wsum = torch.zeros(g, dtype=torch.float32)
    count = torch.zeros(g, dtype=torch.int64)
    for k in range(int(n_chunks.max()) if g else 0):         # a group's partials in chunk order
        live = torch.nonzero(n_chunks > k).reshape(-1)
        total[live] = total[live] + psum[base[live] + k]
        wsum[live] = wsum[live] + pw[base[live] + k]
        count[live] = count[live] + pc[base[live] + k]
    return total, wsum, count


def bank_pool(bank, starts, rows=None, weights=None, normalize=True, n_entries=None, err=None):
    n_entries = rows.shape[0] if rows is not None else int(n_entries)
    return _pool_f32(bank.float(), torch.ones(bank.shape[0]), starts, rows, weights, normalize, n_entries, err)


def bank_pool_fp8(codes, exps, starts, rows=None, weights=None, normalize=True, n_entries=None, err=None):
    n_entries = rows.shape[0] if rows is not None else int(n_entries)
    c = f8.code_values().float()[codes.long()]
    return _pool_f32(c, torch.ldexp(torch.ones(exps.shape[0]), exps.int()), starts, rows, weights, normalize, n_entries, err)


# ------------------------------------------------------------------------------------------------------ from_objects
def objects_csr(point_object, offsets, q_n, m):
    """(starts, rows) of the groups ((scene * Q) + q) * M + rank, bank rows ascending: plain loops over point_object [N, Q]."""
    po = point_object.cpu().tolist()
    s_n = len(offsets) - 1
    groups = [[] for _ in range(s_n * q_n * m)]
    for s in range(s_n):
        for p in range(int(offsets[s]), int(offsets[s + 1])):
            for q in range(q_n):
                if po[p][q] >= 0:
                    groups[(s * q_n + q) * m + po[p][q]].append(p)
    starts = [0]
    for grp in groups:
        starts.append(starts[-1] + len(grp))
    return torch.tensor(starts, dtype=torch.int64), torch.tensor([p for grp in groups for p in grp], dtype=torch.int64)


# ------------------------------------------------------------------------------------------------------ bound cases
C = CHUNK
LENGTHS = (0, 1, C - 1, C, C + 1, 5 * C + 3)
# one and two load groups per lane of an fp16 row (8, 24, 512 | 520, 768, 1024 = BANK_POOL_MAX_DIM), one of an fp8 row (16, 528,
# 768, 1024): every instantiation of the kernel, each up to the widest row it takes
DIMS = {"fp16": (8, 24, 512, 520, 768, 1024), "fp8": (16, 528, 768, 1024)}
# (scaled rows, weights, normalize)
VARIANTS = {"plain": (False, False, True), "weighted": (True, True, True), "raw": (True, True, False), "raw_plain": (False, False, False)}


def _rows_fp16(n, d, gen, scaled):
    x = unit_rows(n, d, gen)
    if scaled:
        x = (x * torch.pow(10.0, 6 * torch.rand(n, 1, generator=gen) - 3)).clamp(-65504, 65504)
    return x.half()


def _weights(n, gen):
    w = 2 * torch.rand(n, generator=gen)
    w[torch.rand(n, generator=gen) < 0.1] = 0
    return w


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
    """-> dict(kind, scenes (fp16 row matrices, one per scene of the bank), starts, rows or None, weights or None, normalize)."""
    kind, d, variant = name.split("-")
    d = int(d)
    gen = torch.Generator().manual_seed(sum(ord(ch) for ch in name))
    if variant in VARIANTS:
        scaled, weighted, normalize = VARIANTS[variant]
        lengths, n = list(LENGTHS), 700
    elif variant == "many":                                  # 300 groups, more than half of them empty
        scaled, weighted, normalize = False, True, True
        lengths = [0] * 300
        for g in torch.randperm(300, generator=gen)[:120].tolist():
            lengths[g] = int(torch.randint(1, 40, (1,), generator=gen))
        lengths[7], lengths[299], n = C + 9, 2 * C, 500
    elif variant == "none":                                  # no entry at all
        scaled, weighted, normalize, lengths, n = False, True, True, [0, 0, 0], 40
    else:                                                    # scene ranges: no index array, the middle scene empty
        scaled, weighted, normalize = False, False, True
        sizes = [C + 5, 0, 40]
        return {"kind": kind, "scenes": [_rows_fp16(m, d, gen, scaled) for m in sizes], "starts": _csr(sizes), "rows": None,
                "weights": None, "normalize": normalize}
    total = sum(lengths)
    return {"kind": kind, "scenes": [_rows_fp16(n, d, gen, scaled)], "starts": _csr(lengths),
            "rows": torch.randint(0, n, (total,), generator=gen), "weights": _weights(total, gen) if weighted else None,
            "normalize": normalize}


# ------------------------------------------------------------------------------------------------------ planted scenes
PLANT_DIM = 64
PLANT_VOXEL = 0.1
PLANT_THRESHOLD = 0.5
PLANT_A_CLUSTERS = (5, 3, 1)     # of 8 clusters per scene: class A's planted share falls from scene to scene
PLANT_CLUSTERS = 8
PLANT_POINTS = 250               # per cluster


@functools.lru_cache(maxsize=None)
def planted(seed=11):
    """Three scenes of 8 clusters x 250 points: a cluster fills a cube of 4^3 voxels, the cubes stand a metre apart; a point's
    feature is its cluster's class direction (A or B, orthonormal) plus Gaussian noise.
    -> dict(feats [fp16 per scene], xyz [float32 per scene], a, b (unit directions, float32), is_a [bool per scene, per point])"""
    gen = torch.Generator().manual_seed(seed)
    a = torch.nn.functional.normalize(torch.randn(PLANT_DIM, generator=gen), dim=0)
    b = torch.randn(PLANT_DIM, generator=gen)
    b = torch.nn.functional.normalize(b - (b @ a) * a, dim=0)
    feats, xyz, is_a = [], [], []
    for n_a in PLANT_A_CLUSTERS:
        order = torch.randperm(PLANT_CLUSTERS, generator=gen)
        f, p, m = [], [], []
        for c in range(PLANT_CLUSTERS):
            cls_a = bool(order[c] < n_a)
            corner = torch.tensor([float(c % 4), float(c // 4), 0.0]) + 0.05
            p.append(corner + 0.4 * torch.rand(PLANT_POINTS, 3, generator=gen))
            scale = 0.5 + 1.5 * torch.rand(PLANT_POINTS, 1, generator=gen)
            f.append(scale * ((a if cls_a else b) + 0.05 * torch.randn(PLANT_POINTS, PLANT_DIM, generator=gen)))
            m.append(torch.full((PLANT_POINTS,), cls_a))
        shuffle = torch.randperm(PLANT_CLUSTERS * PLANT_POINTS, generator=gen)
        feats.append(torch.cat(f)[shuffle].half())
        xyz.append(torch.cat(p)[shuffle].float())
        is_a.append(torch.cat(m)[shuffle])
    return {"feats": feats, "xyz": xyz, "a": a, "b": b, "is_a": is_a}


@functools.lru_cache(maxsize=None)
def planted_reference_route():
    """Find, describe, search again on the planted scenes with the CPU references only (search_reference, objects_reference,
    pool_f64).  -> dict(heat1, heat2, q2 (the best object's descriptor as a query), counts2 and n_objects2 per scene,
    top_is_a (is every scene's top object of the second search a class-A cluster), scene_scores (scene descriptors x (a, b)))"""
    import objects_reference as oref
    import search_reference as sr
    p = planted()
    bank = torch.cat(p["feats"])
    xyz = torch.cat(p["xyz"])
    offsets = [0]
    for f in p["feats"]:
        offsets.append(offsets[-1] + f.shape[0])
    off_t = torch.tensor(offsets, dtype=torch.int64)
    thr = torch.tensor([PLANT_THRESHOLD])
    m = 8

    def find(query):
        heat, _, _, counts = sr.bank_search(bank, off_t, query, thresholds=thr, want_heat=True)
        return heat, counts, oref.find_objects(xyz, offsets, heat, [PLANT_THRESHOLD], voxel_size=PLANT_VOXEL, max_objects=m)

    heat1, _, obj1 = find(p["a"].half()[None])
    starts, rows = objects_csr(obj1["point_object"], offsets, 1, m)
    total, _, wsum, _ = pool_f64(bank.float(), starts, rows, None, True)
    peaks = obj1["peak_score"][:, 0, 0].float().tolist()
    best = peaks.index(max(peaks))                            # the first scene that attains the best peak
    mean = total[best * m] / wsum[best * m]
    q2 = (mean / mean.norm()).half()
    heat2, counts2, obj2 = find(q2[None])
    is_a = torch.cat(p["is_a"])
    top_is_a = [bool(is_a[offsets[s] + int(obj2["peak_point"][s, 0, 0])]) for s in range(3)]
    s_total, _, s_wsum, _ = pool_f64(bank.float(), off_t, None, None, True)
    s_mean = s_total / s_wsum[:, None]
    s_q = (s_mean / s_mean.norm(dim=-1, keepdim=True)).half().double()
    return {"heat1": heat1, "heat2": heat2, "q2": q2, "counts2": counts2[:, 0].tolist(), "n_objects2": obj2["n_objects"][:, 0].tolist(),
            "top_is_a": top_is_a, "scene_scores": (s_q @ torch.stack([p["a"], p["b"]]).double().t()).tolist()}
