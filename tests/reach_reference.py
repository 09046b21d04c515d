"""numpy restatement of openscene_amd.reach and of the second stage `reach=` of openscene_amd.neighbors: the definitions written
literally -- a brute-force minimum of the 64-bit key  d2 << 32 | id  over ALL sources (int64 arithmetic throughout, no 8^3
blocks, no culling), the second stage on top of tests/neighbors_reference.py (imported, not edited) -- the inputs the CPU and
the GPU tests share, and a CPU stand-in for ops.reach_nearest that follows the kernel's contract (host-logic tests only)."""
import itertools

import numpy as np
import torch

import neighbors_reference as nr

F32 = np.float32
NONE = np.iinfo(np.int64).max


# ---------------------------------------------------------------------------------------------------- the search
def nearest(query_cells, source_cells, source_ids, reach):
    """-> (nearest int32 [C], dist2 int32 [C]).  Candidates of a query: the sources of its scene with |dx|, |dy|, |dz| <= reach
    and d2 = dx^2 + dy^2 + dz^2 <= reach^2; the result is the minimum of d2 << 32 | id over them; -1, -1 without one."""
    q = np.asarray(query_cells, dtype=np.int64).reshape(-1, 4)
    s = np.asarray(source_cells, dtype=np.int64).reshape(-1, 4)
    ids = np.asarray(source_ids, dtype=np.int64).reshape(-1)
    assert 1 <= reach <= 4096 and (ids >= 0).all() and ids.shape[0] == s.shape[0]
    near, dist2 = np.full(q.shape[0], -1, dtype=np.int32), np.full(q.shape[0], -1, dtype=np.int32)
    if s.shape[0] == 0:
        return near, dist2
    for a in range(0, q.shape[0], 256):
        d = q[a:a + 256, None, 1:] - s[None, :, 1:]                          # int64: 65 532^2 fits
        d2 = (d * d).sum(2)
        ok = (q[a:a + 256, None, 0] == s[None, :, 0]) & (np.abs(d) <= reach).all(2) & (d2 <= reach * reach)
        key = np.where(ok, (d2 << 32) | ids[None, :], NONE).min(1)
        some = key != NONE
        near[a:a + 256] = np.where(some, key & 0xFFFFFFFF, -1)
        dist2[a:a + 256] = np.where(some, key >> 32, -1)
    return near, dist2


def reach_nearest(query_cells, source_cells, source_ids, reach, err=None):
    """CPU stand-in for ops.reach_nearest."""
    near, dist2 = nearest(query_cells.numpy(), source_cells.numpy(), source_ids.numpy(), int(reach))
    return torch.from_numpy(near), torch.from_numpy(dist2)


# ---------------------------------------------------------------------------------------------------- the grid's voxels
def voxels(xyz, offsets, voxel_size):
    """(coords int64 [V, 4] rows (scene, x, y, z) in first-occurrence order -- the rows of a VoxelGrid --, inverse int64 [N])."""
    cell = np.floor(np.asarray(xyz, dtype=F32).astype(np.float64) / voxel_size).astype(np.int64)
    rows = np.concatenate([nr.scene_of_points(offsets)[:, None], cell], 1)
    seen, coords, inverse = {}, [], np.zeros(rows.shape[0], dtype=np.int64)
    for p, r in enumerate(map(tuple, rows)):
        if r not in seen:
            seen[r] = len(coords)
            coords.append(r)
        inverse[p] = seen[r]
    return np.array(coords, dtype=np.int64).reshape(-1, 4), inverse


def source_voxels(inverse, n_voxels, sources=None):
    held = np.zeros(n_voxels, dtype=bool)
    held[inverse if sources is None else inverse[sources]] = True
    return held


def field(xyz, offsets, voxel_size, sources, reach, per_voxel=False):
    """distance_field: (dist2 int32 [V], nearest int32 [V])."""
    coords, inverse = voxels(xyz, offsets, voxel_size)
    held = np.asarray(sources) if per_voxel else source_voxels(inverse, coords.shape[0], sources)
    near, dist2 = nearest(coords, coords[held], np.nonzero(held)[0], reach)
    return dist2, near


def within(dist2, inverse, distance, voxel_size):
    bound = int(np.floor((float(distance) / voxel_size) ** 2))
    return ((dist2 >= 0) & (dist2 <= bound))[inverse]


def near(xyz, offsets, voxel_size, heat, target, anchor, anchor_threshold, distance, reach=None):
    """fp16 [N, 1]: heat[:, target] where the point's voxel is within `distance` of a voxel with an anchor hit, else -inf."""
    reach = max(1, int(np.ceil(distance / voxel_size))) if reach is None else reach
    a = heat[:, anchor].astype(F32)
    hits = np.isfinite(a) & (a >= F32(anchor_threshold))
    dist2, _ = field(xyz, offsets, voxel_size, hits, reach)
    keep = within(dist2, voxels(xyz, offsets, voxel_size)[1], distance, voxel_size)
    return np.where(keep, heat[:, target], np.float16(-np.inf)).astype(np.float16)[:, None]


# ---------------------------------------------------------------------------------------------------- the second stage
def radius_of(voxel_size, reach, radius=None):
    return (reach + 1) * voxel_size if radius is None else radius


def stage2(first, xyz, offsets, voxel_size, query, qscene, k, reach, radius, sources=None, exclude=None):
    """Behind `first` = (idx, dist2, count) of a 27-cell search: every valid query with count 0 gets the k nearest (d2 <=
    float32(radius)^2, ascending (bits of d2, point)) among the source points of the 27 cells around u, the nearest voxel
    that holds a source point within `reach` cells of the query's cell (a tie: the lowest voxel row)."""
    xyz, query = np.asarray(xyz, dtype=F32), np.asarray(query, dtype=F32)
    idx, dist, count = (np.array(x) for x in first)
    m = query.shape[0]
    qscene = np.broadcast_to(np.asarray(qscene, dtype=np.int64), (m,))
    r2 = nr.r2_of(radius)
    coords, inverse = voxels(xyz, offsets, voxel_size)
    held = source_voxels(inverse, coords.shape[0], sources)
    lists = nr.cell_lists(xyz, offsets, voxel_size, sources)
    ok, cell = nr.query_valid(query, qscene, len(offsets) - 1, voxel_size)
    todo = np.nonzero(ok & (count == 0))[0]
    if todo.shape[0] == 0:
        return idx, dist, count
    qcells = np.concatenate([qscene[todo, None], cell[todo].astype(np.int64)], 1)
    u = nearest(qcells, coords[held], np.nonzero(held)[0], reach)[0]
    for q, v in zip(todo, u):
        if v < 0:
            continue
        s, c = int(coords[v, 0]), coords[v, 1:]
        cands = []
        for o in nr.OFFSETS:
            for p in lists.get((s, int(c[0]) + o[0], int(c[1]) + o[1], int(c[2]) + o[2]), ()):
                if exclude is not None and p == exclude[q]:
                    continue
                d2 = nr.d2_f32(query[q], xyz[p])
                if d2 <= r2:
                    cands.append((int(d2.view(np.uint32)), p, d2))
        idx[q], dist[q], count[q] = nr._finish(cands, k)
    return idx, dist, count


def knn(xyz, offsets, voxel_size, query, qscene, k, reach, radius=None, sources=None, exclude=None):
    """PointIndex.knn(..., reach=reach): both stages cut at float32(radius)^2, radius by default (reach + 1) * voxel_size."""
    radius = radius_of(voxel_size, reach, radius)
    first = nr.knn(xyz, offsets, voxel_size, query, qscene, k, radius, sources=sources, exclude=exclude)
    return stage2(first, xyz, offsets, voxel_size, query, qscene, k, reach, radius, sources=sources, exclude=exclude)


def fill_lists(xyz, offsets, voxel_size, seen, k, reach, radius=None):
    """The neighbour lists fill_missing(..., reach=reach) blends, for ALL points: the first stage at today's radius (at most
    voxel_size), the second at `radius` (default (reach + 1) * voxel_size)."""
    scene = nr.scene_of_points(offsets)
    r1 = voxel_size if radius is None or radius > voxel_size else radius
    first = nr.knn(xyz, offsets, voxel_size, xyz, scene, k, r1, sources=seen)
    return first, stage2(first, xyz, offsets, voxel_size, xyz, scene, k, reach, radius_of(voxel_size, reach, radius), sources=seen)


# ---------------------------------------------------------------------------------------------------- the cases
RANDOM_C = (0, 1, 255, 256, 257, 1000)
RANDOM_S = (0, 1, 511, 512, 513, 3000)
REACHES = (1, 2, 7, 8, 9, 64, 4096)


def random_case(c, s, seed=0):
    """Cells random in a 40^3 box around the origin (negative coordinates), three scenes: scene 1 has no sources, scene 2 no
    queries.  Source ids are a permutation, so id order differs from position order."""
    rng = np.random.default_rng(1000 * c + s + seed)
    q = np.concatenate([rng.integers(0, 2, (c, 1)), rng.integers(-20, 20, (c, 3))], 1).astype(np.int32)
    src = np.concatenate([2 * rng.integers(0, 2, (s, 1)), rng.integers(-20, 20, (s, 3))], 1).astype(np.int32)
    return q, src, rng.permutation(s).astype(np.int32)


def rows(scene, cells):
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    return np.concatenate([np.full((cells.shape[0], 1), scene, dtype=np.int64), cells], 1).astype(np.int32)


def block_edge_case():
    """Queries and sources at cells -9, -8, -1, 0, 7, 8 on each axis (both sides of the 8^3 block faces), ids reversed."""
    edge = np.array(list(itertools.product((-9, -8, -1, 0, 7, 8), repeat=3)))
    rng = np.random.default_rng(3)
    src = edge[rng.random(edge.shape[0]) < 0.3]
    return rows(0, edge), rows(0, src), np.arange(src.shape[0])[::-1].astype(np.int32).copy()


def full_block_case():
    """A full 8^3 block (512 sources, cells 0 .. 7) and its neighbour block holding a single source at (8, 3, 3); queries on
    both sides of the face and far out."""
    full = np.array(list(itertools.product(range(8), repeat=3)))
    src = np.concatenate([full, [[8, 3, 3]]], 0)
    q = np.array([[7, 3, 3], [8, 3, 3], [9, 3, 3], [12, 3, 3], [-3, -3, -3], [3, 3, 3], [8, 8, 8], [20, 3, 3]])
    return rows(0, q), rows(0, src), np.random.default_rng(4).permutation(513).astype(np.int32)


def far_block_case():
    """The nearest source lies in a NON-adjacent block while an adjacent block holds a farther one: the query (7, 0, 0) of
    block (0, 0, 0); a source at (16, 0, 0) -- block (2, 0, 0), d2 81 -- and one at (15, 7, 7) -- block (1, 0, 0), d2 162."""
    return rows(0, [[7, 0, 0]]), rows(0, [[15, 7, 7], [16, 0, 0]]), np.array([0, 1], dtype=np.int32)


def hole_case():
    """A planar patch at voxel 0.05, 20 x 10 voxels, 1 500 points jittered inside one voxel layer, with an unseen strip
    0.40 <= x < 0.65: 5 voxels wide.  values fp16 [N, 3]."""
    rng = np.random.default_rng(21)
    xyz = np.stack([rng.uniform(0.0, 1.0, 1500), rng.uniform(0.0, 0.5, 1500), rng.uniform(0.005, 0.045, 1500)], 1).astype(F32)
    seen = ~((xyz[:, 0] >= F32(0.40)) & (xyz[:, 0] < F32(0.65)))
    values = rng.standard_normal((1500, 3)).astype(np.float16)
    holed = np.where(seen[:, None], values, np.float16(0))
    return dict(xyz=xyz, offsets=[0, 1500], voxel_size=0.05, seen=seen, values=values, holed=holed, reach=8, k=4)


def icp_case():
    """B: a jittered plane z in [0.01, 0.04) at voxel 0.05 (800 points over 1 m x 1 m); A: B shifted 3 voxel sizes along the
    normal.  The 27 cells around every point of A (z cells 2 .. 4) hold no point of B (z cell 0)."""
    rng = np.random.default_rng(22)
    b = np.stack([rng.uniform(0.0, 1.0, 800), rng.uniform(0.0, 1.0, 800), rng.uniform(0.01, 0.04, 800)], 1).astype(F32)
    a = (b + np.array([0.0, 0.0, 0.15], dtype=F32)).astype(F32)
    return dict(a=a, b=b, voxel_size=0.05, reach=4)


def near_case():
    """Two scenes of 600 points in a 1 m x 1 m x 0.1 m slab at voxel 0.05; column 1 (the anchor) is hot inside a 0.1 m disc,
    column 0 (the target) is random; some anchor scores are NaN or +inf."""
    rng = np.random.default_rng(23)
    xyz = np.stack([rng.uniform(0.0, 1.0, 1200), rng.uniform(0.0, 1.0, 1200), rng.uniform(0.0, 0.1, 1200)], 1).astype(F32)
    hot = np.hypot(xyz[:, 0] - F32(0.3), xyz[:, 1] - F32(0.3)) < 0.1
    hot[600:] &= xyz[600:, 0] < F32(0.3)
    anchor = np.where(hot, 0.9, 0.1)
    anchor[::97] = np.nan
    anchor[5::113] = np.inf
    heat = np.stack([rng.random(1200), anchor], 1).astype(np.float16)
    return dict(xyz=xyz, offsets=[0, 600, 1200], voxel_size=0.05, heat=heat, target=0, anchor=1, threshold=0.5, distance=0.2)
