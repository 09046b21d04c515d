"""What the region tests compare against (openscene_amd.regions, csrc/regions.hip), restated independently of the library:

    self_map        the 3^3 neighbour table of a list of (scene, x, y, z) rows, with a dict
    edges_f64       the dot product of every voxel row with its earlier neighbours in float64 on the stored fp16 values,
                    and the per-edge abs-sum  sum |a_c * b_c|
    edges_f32       an independent float32 evaluation: one element after the other, in element order (the kernel deals the
                    elements to 64 lanes and adds the lanes by a butterfly)
    components      union-find over the accepted edges (components_bfs: the same by breadth-first search), the canonical
                    numbering and the min_points rule
    records         the per-region records with integer numpy
    regions_edges, regions_label, regions_records
                    CPU stand-ins with the signatures of the three ops (tests/test_regions_cpu.py)
    edge_case       the inputs the bound is measured on (CPU, edges_f32) and held on (GPU, kernel): the same arrays
    planted         three scenes of touching blobs of six feature prototypes, for the end-to-end tests

sim[i, v] = <vox[v], vox[nbr[k_i, v]]> with k_i = 0 .. 12 (connectivity 26) or 4, 10, 12 (connectivity 6); an absent
neighbour (or one outside the table) gives -inf.  Voxels v and u are joined iff float32(sim) >= float32(threshold)."""
import functools
from collections import deque

import numpy as np
import torch

# The bound of the kernel's sims:  |sim - edges_f64| <= SIM_C * abs-sum + 1e-37  per element, nothing left out.
# SIM_MEASURED_RATIO is the worst error / abs-sum of edges_f32 against edges_f64 over every edge_case
# (tests/test_regions_cpu.py::test_the_bound_constant_is_four_times_the_sequential_sums_worst_ratio measures it again and holds
# the constant to it).  edges_f32 adds the d exact products one after the other -- the longest chain d allows; the kernel
# adds 8 or 16 per lane and then six butterfly levels.  SIM_C = 4 x measured; it must stay at or below SIM_C_CAP, the classical
# bound for d - 1 = 1023 fp32 additions of exact products, which needs no measurement.
# The record is the measurement rounded up in its third digit (1.7403e-7 at 768-special, connectivity 26; elementwise float32
# products added one by one: the same bits on every IEEE host).
SIM_MEASURED_RATIO = 1.75e-7
SIM_C = 4 * SIM_MEASURED_RATIO
SIM_C_CAP = (1024 - 1) * 2.0 ** -24

FACES = (4, 10, 12)              # -z, -y, -x among k = ix + 3 iy + 9 iz


def offsets_of(connectivity):
    assert connectivity in (6, 26)
    return list(range(13)) if connectivity == 26 else list(FACES)


def self_map(coords4):
    """int32 [27, V]: row of the voxel at coords4[v] + offset k (k = ix + 3 iy + 9 iz, each in 0 .. 2 for -1 .. +1) in the same scene, or -1."""
    rows = np.asarray(coords4, dtype=np.int64).tolist()
    index = {tuple(r): i for i, r in enumerate(rows)}
    assert len(index) == len(rows)
    nbr = np.full((27, len(rows)), -1, dtype=np.int32)
    for k in range(27):
        dx, dy, dz = k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1
        for v, (s, x, y, z) in enumerate(rows):
            nbr[k, v] = index.get((s, x + dx, y + dy, z + dz), -1)
    return nbr


# ------------------------------------------------------------------------------------------------------ edges
def _pairs(nbr, connectivity):
    nbr = np.asarray(nbr)
    v_n = nbr.shape[1]
    u = nbr[offsets_of(connectivity)].astype(np.int64)                       # [n_off, V]
    return u, (u >= 0) & (u < v_n)


def edges_f64(vox, nbr, connectivity):
    """vox fp16 [V, d] (torch); nbr int [27, V] -> (sim float64 [n_off, V], abs-sum float64 [n_off, V]) as numpy;
    -inf (abs-sum 0) where there is no neighbour; NaN where either row holds one."""
    x = vox.detach().cpu().double().numpy()
    u, ok = _pairs(nbr, connectivity)
    sim = np.full(u.shape, -np.inf)
    bound = np.zeros(u.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(u.shape[0]):
            v = np.nonzero(ok[i])[0]
            prod = x[v] * x[u[i, v]]
            sim[i, v] = prod.sum(1)
            bound[i, v] = np.abs(prod).sum(1)
    return sim, bound


def edges_f32(vox, nbr, connectivity):
    """float32 [n_off, V] (numpy): the products added one element after the other, in float32."""
    x = vox.detach().cpu().float().numpy()
    u, ok = _pairs(nbr, connectivity)
    sim = np.full(u.shape, -np.inf, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(u.shape[0]):
            v = np.nonzero(ok[i])[0]
            a, b = x[v], x[u[i, v]]
            acc = np.zeros(v.shape[0], dtype=np.float32)
            for c in range(x.shape[1]):
                acc = acc + a[:, c] * b[:, c]                                # (float32 * float32 of fp16 values: exact)
            sim[i, v] = acc
    return sim


def sim_errors(got, want, bound, c):
    """(worst err / abs-sum over the finite elements, elements beyond c * abs-sum + 1e-37, -inf / NaN positions that differ)."""
    got = np.asarray(got, dtype=np.float64)
    fin = np.isfinite(want)
    odd = int((np.isnan(got) != np.isnan(want)).sum() + ((got == -np.inf) != (want == -np.inf)).sum()
              + (np.isfinite(got) != fin).sum())
    err = np.abs(got[fin] - want[fin])
    bad = int((~(err <= c * bound[fin] + 1e-37)).sum())
    some = bound[fin] > 0
    ratio = float((err[some] / bound[fin][some]).max()) if some.any() else 0.0
    return ratio, bad, odd


# ------------------------------------------------------------------------------------------------------ components
def _accepted(sim, nbr, threshold, connectivity):
    """[(v, u)] of the accepted edges: float32 comparison, NaN and -inf never pass."""
    s32 = np.asarray(sim).astype(np.float32)
    u, ok = _pairs(nbr, connectivity)
    with np.errstate(invalid="ignore"):
        take = ok & (s32 >= np.float32(threshold))
    i, v = np.nonzero(take)
    return list(zip(v.tolist(), u[i, v].tolist()))


def _number(root, points_per_voxel, min_points):
    """root int [V] (any representative per component) -> (voxel_root: the smallest row, voxel_region, R): regions numbered
    in ascending order of their smallest row, those with fewer than min_points points dropped (-1)."""
    v_n = len(root)
    smallest = {}
    for v in range(v_n):                                                     # ascending: the first row met is the smallest
        smallest.setdefault(root[v], v)
    voxel_root = np.array([smallest[root[v]] for v in range(v_n)], dtype=np.int32).reshape(v_n)
    ppv = np.ones(v_n, dtype=np.int64) if points_per_voxel is None else np.asarray(points_per_voxel, dtype=np.int64)
    pts = np.zeros(v_n, dtype=np.int64)
    np.add.at(pts, voxel_root, ppv)
    number, r = {}, 0
    for v in range(v_n):
        if voxel_root[v] == v and pts[v] >= min_points:
            number[v] = r
            r += 1
    voxel_region = np.array([number.get(int(voxel_root[v]), -1) for v in range(v_n)], dtype=np.int32).reshape(v_n)
    return voxel_root, voxel_region, r


def components(sim, nbr, threshold, connectivity, points_per_voxel=None, min_points=1):
    """-> (voxel_root int32 [V], voxel_region int32 [V], R) by union-find with path compression."""
    v_n = np.asarray(nbr).shape[1]
    parent = list(range(v_n))

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r

    for v, u in _accepted(sim, nbr, threshold, connectivity):
        a, b = find(v), find(u)
        if a != b:
            parent[a] = b                                                    # (any hook: the numbering below is canonical)
    return _number([find(v) for v in range(v_n)], points_per_voxel, min_points)


def components_bfs(sim, nbr, threshold, connectivity, points_per_voxel=None, min_points=1):
    v_n = np.asarray(nbr).shape[1]
    adj = [[] for _ in range(v_n)]
    for v, u in _accepted(sim, nbr, threshold, connectivity):
        adj[v].append(u)
        adj[u].append(v)
    root = [-1] * v_n
    for s in range(v_n):
        if root[s] >= 0:
            continue
        root[s] = s
        todo = deque([s])
        while todo:
            a = todo.popleft()
            for b in adj[a]:
                if root[b] < 0:
                    root[b] = s
                    todo.append(b)
    return _number(root, points_per_voxel, min_points)


def canonical(labels):
    """A labelling [N] (-1: none) as a partition: every label replaced by the first index that carries it."""
    first = {}
    out = []
    for i, r in enumerate(np.asarray(labels).tolist()):
        out.append(-1 if r < 0 else first.setdefault(r, i))
    return out


# ------------------------------------------------------------------------------------------------------ records
def records(voxel_region, n_regions, xyz, inverse, coords4):
    """dict of numpy arrays like ops.regions_records': python / numpy integers, float32 min / max.  Entries out of range are skipped."""
    region = np.asarray(voxel_region).astype(np.int64)
    inv = np.asarray(inverse).astype(np.int64)
    c4 = np.asarray(coords4).astype(np.int64)
    x32 = np.asarray(xyz, dtype=np.float32)
    r_n, v_n = int(n_regions), region.shape[0]
    out = {"n_points": np.zeros(r_n, np.int64), "n_voxels": np.zeros(r_n, np.int64), "vox_sum": np.zeros((r_n, 3), np.int64),
           "box_min": np.zeros((r_n, 3), np.float32), "box_max": np.zeros((r_n, 3), np.float32), "scene": np.full(r_n, -1, np.int32)}
    okv = (region >= 0) & (region < r_n)
    for v in np.nonzero(okv)[0][::-1]:                                      # descending: the smallest row writes last
        out["scene"][region[v]] = c4[v, 0]
    np.add.at(out["n_voxels"], region[okv], 1)
    okp = (inv >= 0) & (inv < v_n)
    pr = np.where(okp, region[np.clip(inv, 0, max(v_n - 1, 0))] if v_n else -1, -1)
    okp &= (pr >= 0) & (pr < r_n)
    p = np.nonzero(okp)[0]
    np.add.at(out["n_points"], pr[p], 1)
    np.add.at(out["vox_sum"], pr[p], c4[inv[p], 1:])
    lo = np.full((r_n, 3), np.inf, np.float32)
    hi = np.full((r_n, 3), -np.inf, np.float32)
    np.minimum.at(lo, pr[p], x32[p])
    np.maximum.at(hi, pr[p], x32[p])
    some = out["n_points"] > 0
    out["box_min"][some] = lo[some]
    out["box_max"][some] = hi[some]
    return out


RECORD_FIELDS = ("scene", "n_points", "n_voxels", "vox_sum", "box_min", "box_max")


def assert_records(got, want):
    """Every field of a RegionResult (or an ops dict) against records(): exact."""
    for f in RECORD_FIELDS:
        g = (got[f] if isinstance(got, dict) else getattr(got, f)).cpu()
        w = torch.from_numpy(want[f])
        assert g.dtype == w.dtype and g.shape == w.shape, (f, g.dtype, g.shape, w.dtype, w.shape)
        assert bool((g == w).all()), (f, g[g != w][:8], w[g != w][:8])     # (-0 == +0 in the boxes)


# ------------------------------------------------------------------------------------------------------ stand-ins
def _err_bits(err, bits):
    if bits:
        if err is None:
            raise RuntimeError("regions: err bits %d" % bits)
        err |= bits


def regions_edges(vox, nbr, connectivity=26, err=None):
    n = nbr.numpy()
    _err_bits(err, 1 if bool((n[offsets_of(connectivity)] >= n.shape[1]).any()) else 0)
    return torch.from_numpy(edges_f32(vox, n, connectivity))


def regions_label(sim, nbr, connectivity=26, threshold=0.9, err=None):
    n = nbr.numpy()
    _err_bits(err, 1 if bool((n[offsets_of(connectivity)] >= n.shape[1]).any()) else 0)
    return torch.from_numpy(components(sim.numpy(), n, threshold, connectivity)[0])


def regions_records(voxel_region, n_regions, xyz, inverse, coords4, err=None):
    region, inv = voxel_region.numpy(), inverse.numpy()
    bits = 2 if bool(((inv < 0) | (inv >= region.shape[0])).any()) else 0
    bits |= 4 if bool(((region < -1) | (region >= int(n_regions))).any()) else 0
    _err_bits(err, bits)
    return {k: torch.from_numpy(a) for k, a in records(region, n_regions, xyz.numpy(), inv, coords4.numpy()).items()}


# ------------------------------------------------------------------------------------------------------ edge cases
EDGE_DIMS = (8, 24, 520, 768, 1024)      # one vector load, fewer loads than lanes, not a multiple of 64 * 8, the workload's width, the limit
EDGE_SPECIAL = (24, 768)                 # the widths that also run with subnormals, scaled rows, a NaN row and a zero row


def edge_case_names():
    return ["%d-plain" % d for d in EDGE_DIMS] + ["%d-special" % d for d in EDGE_SPECIAL]


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """-> dict(vox fp16 [V, d], nbr int32 [27, V] (numpy), coords4, isolated, nan_row, zero_row (rows or None)).
    A few hundred voxels: a dense 4^3 corner (26 neighbours inside), random cells of a 12^3 box, one voxel far away."""
    d, variant = name.split("-")
    d = int(d)
    gen = torch.Generator().manual_seed(1000 + d + (7 if variant == "special" else 0))
    box = torch.randperm(12 ** 3, generator=gen)[:330].tolist()
    cells = {(x, y, z) for x in range(4) for y in range(4) for z in range(4)}
    cells |= {(c % 12, (c // 12) % 12, c // 144) for c in box}
    cells = sorted(cells)
    order = torch.randperm(len(cells), generator=gen).tolist()
    cells = [cells[i] for i in order] + [(40, 40, 40)]
    coords4 = np.array([(0,) + c for c in cells], dtype=np.int32)
    v_n = len(cells)
    vox = torch.nn.functional.normalize(torch.randn(v_n, d, generator=gen), dim=1).half()
    nan_row = zero_row = None
    if variant == "special":
        rows = torch.randperm(v_n - 1, generator=gen)[:12].tolist()
        for r in rows[:6]:                                                   # rows scaled by 2^-10: most elements become fp16 subnormals
            vox[r] = (vox[r].float() * 2.0 ** -10).half()
        for r in rows[6:10]:                                                 # a few subnormal elements in ordinary rows
            cols = torch.randperm(d, generator=gen)[:3]
            vox[r, cols] = torch.tensor([2.0 ** -24, -3 * 2.0 ** -24, 1023 * 2.0 ** -24]).half()
        nan_row, zero_row = rows[10], rows[11]
        vox[nan_row, d // 2] = float("nan")
        vox[zero_row] = 0
    return {"vox": vox, "nbr": self_map(coords4), "coords4": coords4, "isolated": v_n - 1, "nan_row": nan_row, "zero_row": zero_row}


# ------------------------------------------------------------------------------------------------------ planted scenes
PLANT_DIM = 64
PLANT_VOXEL = 0.1
PLANT_SIMILARITY = 0.7
PLANT_MARGIN = 1e-3              # no reference sim this close to the threshold: > 16 x SIM_C_CAP for unit rows (abs-sum <= 1)
PLANT_PROTOTYPES = 6
PLANT_SIDE = 4                   # a blob fills a cube of 4^3 voxels
PLANT_POINTS = 3                 # per voxel


@functools.lru_cache(maxsize=None)
def planted(seed=23):
    """Three scenes of six touching blobs: cubes of 4^3 voxels in a 3 x 2 block, face to face, every blob of a scene with its
    own prototype (six orthonormal directions), every voxel with three points; a point's feature is its blob's prototype plus
    small Gaussian noise, scaled over U(0.5, 2).  The points of a scene are shuffled.
    -> dict(feats [fp16 per scene], xyz [float32 per scene], protos float32 [6, dim], cls [int64 per scene, per point])"""
    gen = torch.Generator().manual_seed(seed)
    protos = torch.linalg.qr(torch.randn(PLANT_DIM, PLANT_PROTOTYPES, generator=gen))[0].t().contiguous()
    feats, xyz, cls = [], [], []
    side = PLANT_SIDE
    for s in range(3):
        assign = torch.randperm(PLANT_PROTOTYPES, generator=gen).tolist()
        f, p, c = [], [], []
        for b in range(6):
            corner = torch.tensor([(b % 3) * side, (b // 3) * side, 0], dtype=torch.float32)
            cell = torch.tensor([(x, y, z) for x in range(side) for y in range(side) for z in range(side)], dtype=torch.float32)
            cell = (cell + corner).repeat_interleave(PLANT_POINTS, 0)
            n = cell.shape[0]
            p.append((cell + 0.1 + 0.8 * torch.rand(n, 3, generator=gen)) * PLANT_VOXEL)
            scale = 0.5 + 1.5 * torch.rand(n, 1, generator=gen)
            f.append(scale * (protos[assign[b]] + 0.03 * torch.randn(n, PLANT_DIM, generator=gen)))
            c.append(torch.full((n,), assign[b], dtype=torch.int64))
        shuffle = torch.randperm(6 * side ** 3 * PLANT_POINTS, generator=gen)
        feats.append(torch.cat(f)[shuffle].half())
        xyz.append(torch.cat(p)[shuffle].float())
        cls.append(torch.cat(c)[shuffle])
    return {"feats": feats, "xyz": xyz, "protos": protos, "cls": cls}


def planted_check(graph, result, cls):
    """The end-to-end claims on a SimilarityGraph / RegionResult of the planted scenes (any device): the margin condition on
    the float64 sims of the graph's own rows, the partition of the float64 reference, pure regions.  -> the class per region"""
    grid = graph.grid
    nbr = grid.nbr.cpu().numpy()
    sim64, _ = edges_f64(graph.vox, nbr, grid.connectivity)
    fin = np.isfinite(sim64)
    assert fin.sum() > 0 and float(np.abs(sim64[fin] - PLANT_SIMILARITY).min()) > PLANT_MARGIN
    _, region, r = components(sim64, nbr, PLANT_SIMILARITY, grid.connectivity)
    assert r == result.n_regions == 3 * PLANT_PROTOTYPES
    assert np.array_equal(result.voxel_region.cpu().numpy(), region)
    pr = result.point_region.cpu()
    assert int(pr.min()) >= 0 and torch.equal(pr.long(), torch.from_numpy(region).long()[grid.inverse.cpu().long()])
    cls = torch.cat(cls)
    want = torch.full((r,), -1, dtype=torch.int64)
    want[pr.long()] = cls
    assert torch.equal(want[pr.long()], cls)                                 # every region holds one class only
    return want
