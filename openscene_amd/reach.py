"""Nearest sources at any range: exact distance fields on the voxel grid.

Every spatial operation of openscene_amd.neighbors stops one voxel from the query: 27 cells hold no more.  Holes wider than a
voxel, a mesh vertex more than a cell from the bank, a wall displaced by three voxels, and every question that relates two
results in space -- "the lamp near the sofa", "mugs within a metre of the sink" -- need the distance from every voxel to the
nearest voxel of a set, tens of cells away.  One primitive answers them:

    for every query cell the nearest source cell of the same scene inside a Euclidean ball of `reach` cells

On the integer lattice the squared distance d2 = dx^2 + dy^2 + dz^2 is an integer, the result is the minimum of one 64-bit key
uint32(d2) << 32 | uint32(voxel row) over the candidates (|dx|, |dy|, |dz| <= reach and d2 <= reach^2), and so it is defined
bit for bit whatever the schedule: a tie goes to the lowest voxel row.  Kernel: csrc/reach.hip through ops.reach_nearest; no
CPU path.

    distance_field(grid, sources, reach)   -> DistanceField: dist2, nearest per voxel; .distance() .at_points() .within()
    nearest_voxel(grid, xyz, scene, ...)   the same for foreign positions
    near(grid, heat, target, anchor, ...)  a heat-map column kept where an anchor column's hits are near: "A near B"

The second stage `reach=` of PointIndex.knn / knn_self, transfer, fill_missing and align.refine_icp is built on the same
primitive (openscene_amd.neighbors.PointIndex._stage2).
"""
import math

import torch

from . import ops
from .objects import COORD_LIMIT, VoxelGrid


def _source_voxels(grid, sources, per_voxel):
    """bool [V]: the voxels that are sources."""
    if not isinstance(grid, VoxelGrid):
        raise TypeError("grid must be a VoxelGrid")
    if not isinstance(sources, torch.Tensor) or sources.dtype != torch.bool:
        raise TypeError("sources must be a bool tensor")
    want = grid.n_voxels if per_voxel else grid.n_points
    if tuple(sources.shape) != (want,) or sources.device != grid.device:
        raise ValueError("sources must be a bool [%d] mask over the grid's %s on the grid's device" % (want, "voxels" if per_voxel else "points"))
    if per_voxel:
        return sources
    held = torch.zeros(grid.n_voxels, dtype=torch.bool, device=grid.device)
    held[grid.inverse.long()[sources]] = True
    return held


def _search(grid, cells, held, reach):
    rows = torch.nonzero(held).reshape(-1)
    return ops.reach_nearest(cells, grid.coords[rows].contiguous(), rows.to(torch.int32).contiguous(), reach)


class DistanceField:
    """Per voxel of `grid` the nearest source voxel within `reach` cells: dist2 int32 [V] (cells squared), nearest int32 [V] (the
    source's voxel row); both -1 where no source lies within reach."""

    def __init__(self, grid, dist2, nearest, reach):
        self.grid, self.dist2, self.nearest, self.reach = grid, dist2, nearest, reach

    def distance(self):
        """float32 [V]: sqrt(float32(dist2)) * voxel_size, +inf where there is no source within reach."""
        d = torch.sqrt(self.dist2.clamp(min=0).float()) * self.grid.voxel_size
        return torch.where(self.dist2 >= 0, d, torch.full_like(d, float("inf")))

    def at_points(self):
        """float32 [N]: distance() of every point's voxel."""
        return self.distance()[self.grid.inverse.long()]

    def within(self, distance):
        """bool [N]: the points whose voxel lies within `distance` (metres, between cells) of a source voxel.  Decided on
        integers: dist2 <= floor((distance / voxel_size)^2), the bound computed once on the host in float64."""
        distance = float(distance)
        if not distance >= 0.0:
            raise ValueError("distance must be >= 0 (got %r)" % (distance,))
        bound = min(math.floor((distance / self.grid.voxel_size) ** 2), 2 ** 31 - 1)
        return ((self.dist2 >= 0) & (self.dist2 <= bound))[self.grid.inverse.long()]


def distance_field(grid, sources, reach, per_voxel=False):
    """The distance from every voxel of `grid` to the nearest source voxel of its scene within `reach` (1 .. 4096) cells.
    sources bool [N]: a voxel is a source when it holds a source point; with per_voxel a bool [V] mask over the voxel rows.
    -> DistanceField.  Exact: integers only, a tie goes to the lowest voxel row; a source voxel has dist2 0 and itself."""
    held = _source_voxels(grid, sources, per_voxel)
    reach = ops.reach_value(reach)
    nearest, dist2 = _search(grid, grid.coords, held, reach)
    return DistanceField(grid, dist2, nearest, reach)


def nearest_voxel(grid, query_xyz, scene, sources, reach, per_voxel=False):
    """For foreign positions: (nearest int32 [M], dist2 int32 [M]) -- the source voxel row nearest to the cell
    floor(xyz.double() / voxel_size) of every query within `reach` cells of it, and the squared distance in cells; -1, -1
    without one.  query_xyz float [M, 3]; scene an int or int64 [M].  A query with a non-finite coordinate, a cell outside
    the packable range or a scene outside [0, S) is invalid and gets -1, -1."""
    held = _source_voxels(grid, sources, per_voxel)
    reach = ops.reach_value(reach)
    dev = grid.device
    if not isinstance(query_xyz, torch.Tensor) or not query_xyz.dtype.is_floating_point:
        raise TypeError("query_xyz must be a float tensor")
    if query_xyz.dim() != 2 or query_xyz.shape[1] != 3:
        raise ValueError("query_xyz must be [M, 3] (got %s)" % (tuple(query_xyz.shape),))
    if query_xyz.device != dev:
        raise ValueError("query_xyz must be on the grid's device (%s, got %s)" % (dev, query_xyz.device))
    m = query_xyz.shape[0]
    if isinstance(scene, torch.Tensor):
        if scene.dtype != torch.int64:
            raise TypeError("scene must be an int or an int64 tensor")
        if tuple(scene.shape) != (m,) or scene.device != dev:
            raise ValueError("scene must be an int64 [%d] vector on the grid's device" % m)
    else:
        scene = torch.full((m,), int(scene), dtype=torch.int64, device=dev)
    cell = torch.floor(query_xyz.detach().float().double() / grid.voxel_size)
    valid = ((cell > -COORD_LIMIT) & (cell < COORD_LIMIT)).all(1) & (scene >= 0) & (scene < grid.n_scenes)      # (NaN and inf fail)
    cells = torch.cat([torch.where(valid, scene, 0)[:, None].to(torch.int32),
                       torch.where(valid[:, None], cell, 0.0).to(torch.int32)], 1).contiguous()
    nearest, dist2 = _search(grid, cells, held, reach)        # (an invalid query rides on cell (0, 0, 0, 0) and is dropped here)
    none = torch.full_like(nearest, -1)
    return torch.where(valid, nearest, none), torch.where(valid, dist2, none)


def near(grid, heat, target, anchor, anchor_threshold, distance, reach=None):
    """"target near anchor" as a heat-map: fp16 [N, 1], heat[:, target] where the point's voxel lies within `distance`
    (metres, between cells) of a voxel holding a point with heat[:, anchor] finite and >= anchor_threshold; -inf elsewhere.
    reach: the cells searched, by default ceil(distance / voxel_size).  find_objects and smooth take the result as it is."""
    if not isinstance(grid, VoxelGrid):
        raise TypeError("grid must be a VoxelGrid")
    if not isinstance(heat, torch.Tensor) or heat.dtype != torch.float16:
        raise TypeError("heat must be a float16 tensor (got %s)" % (heat.dtype if isinstance(heat, torch.Tensor) else type(heat).__name__))
    if heat.dim() != 2 or heat.shape[0] != grid.n_points or heat.shape[1] < 1:
        raise ValueError("heat must be [%d, Q] for this grid (got %s)" % (grid.n_points, tuple(heat.shape)))
    if heat.device != grid.device:
        raise ValueError("heat must be on the grid's device (%s, got %s)" % (grid.device, heat.device))
    target, anchor = int(target), int(anchor)
    for name, col in (("target", target), ("anchor", anchor)):
        if not 0 <= col < heat.shape[1]:
            raise IndexError("%s column %d of %d" % (name, col, heat.shape[1]))
    distance = float(distance)
    if not (distance >= 0.0 and distance != float("inf")):
        raise ValueError("distance must be finite and >= 0 (got %r)" % (distance,))
    if reach is None:
        reach = max(1, math.ceil(distance / grid.voxel_size))
    a = heat[:, anchor].float()
    hits = torch.isfinite(a) & (a >= float(anchor_threshold))
    keep = distance_field(grid, hits, reach).within(distance)
    column = heat[:, target]
    return torch.where(keep, column, torch.full_like(column, float("-inf")))[:, None].contiguous()
