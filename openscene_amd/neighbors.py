"""Spatial neighbours on the voxel grid: move a per-point result to other points.

Every application result -- `search` heat-maps, `find_objects`, `segment`, `pool`, `render` through its point-id image -- is a
tensor over the bank's own points.  Three needs come down to one operation, the k nearest points of a query and a gather
along them:

    points without a fused feature   ``run/evaluate.py:297-300``: "some points do not have 2D features from 2D feature
                                     fusion"; FeatureFusion.finish() returns the point_ids that were seen, io.load_fused_features
                                     the mask.  The rest have zero rows and punch holes into heat-maps.  -> fill_missing
    other point sets                 the full-resolution mesh, a second scan, a click un-projected to 3-D.  -> transfer
    noise                            one stray point over the threshold is one object.  -> smooth

    PointIndex(grid, sources)   the source points of a VoxelGrid per voxel row (a CSR), and the grid's hash table
    .knn / .knn_self            -> Neighbors(idx, dist2, count): the k nearest sources inside the 27 cells around a query
    Neighbors.blend / .vote     the weighted mean of value rows / the majority label along the lists
    transfer, fill_missing, smooth   the three uses above

The candidates of a query are the source points of the 27 cells around its own; with radius <= voxel_size that is the
radius search.  Distances are separately rounded float32 operations, the order is (d2, point index): exact, and bitwise
repeatable.  Kernels: csrc/neighbors.hip through ops.knn_grid / ops.knn_blend / ops.knn_vote; no CPU path.
"""
import numpy as np
import torch

from . import ops
from .objects import COORD_LIMIT, VoxelGrid

WEIGHTS = ("uniform", "inverse")


def _radius(radius, voxel_size, reach=None):
    if reach is None:
        radius = voxel_size if radius is None else float(radius)
        if not 0.0 < radius <= voxel_size:
            raise ValueError("radius must lie in (0, voxel_size = %r] (got %r): 27 cells hold no more" % (voxel_size, radius))
    else:
        limit = (ops.reach_value(reach) + 1) * voxel_size
        radius = limit if radius is None else float(radius)
        if not 0.0 < radius <= limit:
            raise ValueError("radius must lie in (0, (reach + 1) * voxel_size = %r] (got %r)" % (limit, radius))
    r = np.float32(radius)
    return float(r * r)                                      # float32(radius) * float32(radius), one float32 rounding


class Neighbors:
    """The neighbour lists of M queries: idx int32 [M, k] (grid point numbers, -1 past count), dist2 float32 [M, k] (+inf past
    count), count int32 [M]; ascending (dist2, idx).  `index` is the PointIndex that made them."""

    def __init__(self, idx, dist2, count, index):
        self.idx, self.dist2, self.count, self.index = idx, dist2, count, index

    def __iter__(self):                                      # idx, dist2, count = neighbors
        return iter((self.idx, self.dist2, self.count))

    def blend(self, values, weights="uniform", fill=0):
        """(out [M, C], found bool [M]): out[m] = sum_j w_j values[idx[m, j]] / sum_j w_j over j < count[m], in float32, rounded
        once to the type of `values` (fp16 or fp32 [N, C]: a heat-map, a feature matrix).  weights "uniform": w = 1;
        "inverse": w = 1 / (dist2 + eps), eps = float32((1e-3 voxel_size)^2).  count == 0 gives `fill` and found False;
        k = 1 uniform is a bitwise copy of the row."""
        if weights not in WEIGHTS:
            raise ValueError('weights must be "uniform" or "inverse" (got %r)' % (weights,))
        if not isinstance(values, torch.Tensor) or values.dtype not in (torch.float16, torch.float32):
            raise TypeError("values must be a float16 or float32 tensor (got %s)"
                            % (values.dtype if isinstance(values, torch.Tensor) else type(values).__name__))
        n = self.index.grid.n_points
        if values.dim() != 2 or values.shape[0] != n or values.shape[1] < 1:
            raise ValueError("values must be [%d, C] for this grid (got %s)" % (n, tuple(values.shape)))
        if values.device != self.idx.device:
            raise ValueError("values must be on the grid's device (%s, got %s)" % (self.idx.device, values.device))
        eps = float(np.float32((1e-3 * self.index.grid.voxel_size) ** 2))
        return ops.knn_blend(values.contiguous(), self.idx, self.dist2, self.count, inverse=weights == "inverse", eps=eps, fill=fill)

    def vote(self, labels, fill=-1):
        """int64 [M]: the label (int64 [N]; negative ones are ignored) most of a query's neighbours hold; a tie goes to the
        label whose first holder is nearest; `fill` without a labelled neighbour.  Exact."""
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64:
            raise TypeError("labels must be an int64 tensor")
        n = self.index.grid.n_points
        if labels.dim() != 1 or labels.shape[0] != n:
            raise ValueError("labels must be [%d] for this grid (got %s)" % (n, tuple(labels.shape)))
        if labels.device != self.idx.device:
            raise ValueError("labels must be on the grid's device (%s, got %s)" % (self.idx.device, labels.device))
        return ops.knn_vote(labels.contiguous(), self.idx, self.count, fill=fill)


class PointIndex:
    """The source points of a VoxelGrid, listed per voxel row.  sources: bool [N] on the grid's device (None: every point);
    only source points are returned as neighbours.  Holds
        cell_start   int32 [V + 1]                    cell_points  int32 [n_src], ascending point index inside a voxel
        table        the grid's hash table (probed for the cells of foreign queries)
    The CSR is a stable sort of grid.inverse[sources] and a cumulative count: plumbing, in torch."""

    def __init__(self, grid, sources=None):
        if not isinstance(grid, VoxelGrid):
            raise TypeError("grid must be a VoxelGrid")
        n, v, dev = grid.n_points, grid.n_voxels, grid.device
        if sources is None:
            ids = torch.arange(n, device=dev)
        else:
            if not isinstance(sources, torch.Tensor) or sources.dtype != torch.bool:
                raise TypeError("sources must be a bool tensor")
            if tuple(sources.shape) != (n,) or sources.device != dev:
                raise ValueError("sources must be a bool [%d] mask on the grid's device" % n)
            ids = torch.nonzero(sources).reshape(-1)
        self.grid = grid
        self.table = grid.table
        cell = grid.inverse.long()[ids]
        perm = torch.sort(cell, stable=True)[1]
        self.cell_points = ids[perm].to(torch.int32).contiguous()
        start = torch.zeros(v + 1, dtype=torch.int64, device=dev)
        start[1:] = torch.cumsum(torch.bincount(cell, minlength=v), 0)
        self.cell_start = start.to(torch.int32).contiguous()
        self._self_order = self.cell_points if sources is None else None      # all N points in cell order (knn_self)
        self._source_voxels = None                                            # (cells int32 [U, 4], rows int32 [U]): see _stage2

    def _knn(self, nbr, query, q_cell, exclude, order, k, r2):
        g = self.grid
        idx, dist2, count = ops.knn_grid(g.xyz, self.cell_start, self.cell_points, nbr, query, q_cell, k, r2, exclude=exclude, order=order)
        return Neighbors(idx, dist2, count, self)

    def _stage2(self, res, query, cells, column, exclude, k, r2, reach):
        """The second stage behind a 27-cell search, for the queries it left with count 0 (the others keep their rows bit for
        bit).  cells int32 [U, 4] and column int32 [M] (-1: an invalid query) give every query's cell.  Per such query: u, the
        nearest voxel that holds a source point within `reach` cells of the query's cell (ops.reach_nearest: exact, a tie in
        the cell distance goes to the lowest voxel row); then the k nearest among the source points of the 27 cells around u
        (grid.nbr[:, u]) within r2, by ops.knn_grid as in the first stage.  That is the nearest of a STATED CANDIDATE SET --
        the points around the nearest occupied cell -- not the exact metric nearest neighbour: a point of a cell farther
        than u may lie nearer than every candidate."""
        g = self.grid
        rows = torch.nonzero((column >= 0) & (res.count == 0)).reshape(-1)
        if rows.numel() == 0 or g.n_voxels == 0:
            return res
        if self._source_voxels is None:
            held = torch.nonzero(self.cell_start[1:] > self.cell_start[:-1]).reshape(-1)
            self._source_voxels = (g.coords[held].contiguous(), held.to(torch.int32).contiguous())
        used, place = torch.unique(column[rows].long(), return_inverse=True)
        u = ops.reach_nearest(cells[used].contiguous(), self._source_voxels[0], self._source_voxels[1], reach)[0]
        q_cell = u[place].contiguous()
        order = torch.sort(q_cell, stable=True)[1].to(torch.int32).contiguous()
        idx, dist2, count = ops.knn_grid(g.xyz, self.cell_start, self.cell_points, g.nbr, query[rows].contiguous(), q_cell, k, r2,
                                         exclude=None if exclude is None else exclude[rows].contiguous(), order=order)
        res.idx[rows], res.dist2[rows], res.count[rows] = idx, dist2, count
        return res

    def knn(self, query_xyz, k, radius=None, scene=0, exclude=None, reach=None):
        """The k (1 .. 16) nearest source points of every query within `radius` (default and at most voxel_size), among the
        source points of the 27 cells around the query's cell floor(xyz.double() / voxel_size) of its scene.
        query_xyz float [M, 3] (taken as float32); scene an int or int64 [M]; exclude int32 [M]: a point not to return, or
        None.  A query with a non-finite coordinate, a cell outside the packable range or a scene outside [0, S) gets
        count 0.  -> Neighbors

        reach (an int, 1 .. 4096 cells): a second stage for the valid queries the 27 cells leave with count 0 -- the k nearest
        among the source points of the 27 cells around the nearest voxel that holds a source point within `reach` cells of the
        query's cell (_stage2).  `radius` may then be any positive value up to (reach + 1) * voxel_size, its default, and both
        stages cut at float32(radius)^2.  Beyond one voxel this is the nearest of that stated candidate set, NOT the exact
        metric nearest neighbour.  Rows the first stage finds are bit for bit what it returns; without `reach` the call is
        what it was."""
        g = self.grid
        dev = g.device
        if not isinstance(query_xyz, torch.Tensor) or not query_xyz.dtype.is_floating_point:
            raise TypeError("query_xyz must be a float tensor")
        if query_xyz.dim() != 2 or query_xyz.shape[1] != 3:
            raise ValueError("query_xyz must be [M, 3] (got %s)" % (tuple(query_xyz.shape),))
        if query_xyz.device != dev:
            raise ValueError("query_xyz must be on the grid's device (%s, got %s)" % (dev, query_xyz.device))
        k = ops.knn_k(k)
        r2 = _radius(radius, g.voxel_size, reach)
        q = query_xyz.detach().float().contiguous()
        m = q.shape[0]
        if isinstance(scene, torch.Tensor):
            if scene.dtype != torch.int64:
                raise TypeError("scene must be an int or an int64 tensor")
            if tuple(scene.shape) != (m,) or scene.device != dev:
                raise ValueError("scene must be an int64 [%d] vector on the grid's device" % m)
        else:
            scene = torch.full((m,), int(scene), dtype=torch.int64, device=dev)
        if exclude is not None:
            if not isinstance(exclude, torch.Tensor) or exclude.dtype != torch.int32:
                raise TypeError("exclude must be an int32 tensor")
            if tuple(exclude.shape) != (m,) or exclude.device != dev:
                raise ValueError("exclude must be an int32 [%d] vector on the grid's device" % m)
            exclude = exclude.contiguous()
        if reach is None:
            nbr, q_cell, order = self.query_cells(q, scene)
            return self._knn(nbr, q, q_cell, exclude, order, k, r2)
        nbr, q_cell, order, cells = self._query_cells(q, scene)
        return self._stage2(self._knn(nbr, q, q_cell, exclude, order, k, r2), q, cells, q_cell, exclude, k, r2, reach)

    def query_cells(self, q, scene):
        """The cells of foreign queries (q float32 [M, 3], scene int64 [M]) -> (nbr int32 [27, C]: the grid's voxel rows around
        each distinct cell; q_cell int32 [M]: a query's column, -1 when it is invalid; order int32 [M]: the queries sorted by
        column).  Floor in torch, ops.coords_unique over the cells, ops.kmap_build against the grid's table."""
        return self._query_cells(q, scene)[:3]

    def _query_cells(self, q, scene):
        """query_cells and, fourth, the distinct cells themselves: int32 [C, 4] rows (scene, x, y, z)."""
        g = self.grid
        dev, m = g.device, q.shape[0]
        if m == 0 or g.n_voxels == 0:
            return (torch.empty((27, 0), dtype=torch.int32, device=dev), torch.full((m,), -1, dtype=torch.int32, device=dev), None,
                    torch.empty((0, 4), dtype=torch.int32, device=dev))
        cell = torch.floor(q.double() / g.voxel_size)
        valid = ((cell > -COORD_LIMIT) & (cell < COORD_LIMIT)).all(1) & (scene >= 0) & (scene < g.n_scenes)     # (NaN and inf fail)
        coords4 = torch.cat([torch.where(valid, scene, 0)[:, None].to(torch.int32),
                             torch.where(valid[:, None], cell, 0.0).to(torch.int32)], 1).contiguous()
        cells, column, _first, _table = ops.coords_unique(coords4)            # an invalid query rides on cell (0, 0, 0, 0) and is dropped below
        nbr = ops.kmap_build(self.table, cells.contiguous(), 3, 1)
        q_cell = torch.where(valid, column.to(torch.int32), -1).contiguous()
        order = torch.sort(q_cell, stable=True)[1].to(torch.int32).contiguous()
        return nbr.contiguous(), q_cell, order, cells.contiguous()

    def knn_self(self, k, radius=None, include_self=True, reach=None):
        """knn for the grid's own points as queries -- all N of them, not only the sources -- with the cells taken from
        grid.nbr and grid.inverse (no hash probe).  include_self False: a point is not its own neighbour.  `reach`: the second
        stage, as in knn (the nearest of a stated candidate set, not the exact metric nearest neighbour).  -> Neighbors"""
        g = self.grid
        k = ops.knn_k(k)
        r2 = _radius(radius, g.voxel_size, reach)
        if self._self_order is None:
            self._self_order = torch.sort(g.inverse.long(), stable=True)[1].to(torch.int32).contiguous()
        exclude = None if include_self else torch.arange(g.n_points, dtype=torch.int32, device=g.device)
        res = self._knn(g.nbr, g.xyz, g.inverse, exclude, self._self_order, k, r2)
        return res if reach is None else self._stage2(res, g.xyz, g.coords, g.inverse, exclude, k, r2, reach)


def transfer(index, query_xyz, values, k=1, radius=None, weights="uniform", scene=0, fill=0, reach=None):
    """Values of the grid's points at other positions: index.knn(query_xyz, k, radius, scene).blend(values, weights, fill)
    -> (out [M, C], found bool [M]).  A click un-projected to 3-D, the vertices of the full-resolution mesh, a second scan.
    `reach` (cells): knn's second stage for the queries more than a cell from every bank point -- beyond one voxel the
    neighbours are the nearest of a stated candidate set (PointIndex.knn), not the exact metric nearest neighbours."""
    if not isinstance(index, PointIndex):
        raise TypeError("index must be a PointIndex")
    search = dict(radius=radius, scene=scene) if reach is None else dict(radius=radius, scene=scene, reach=reach)
    return index.knn(query_xyz, k, **search).blend(values, weights=weights, fill=fill)


def _values_of(values):
    from .search import FeatureBank
    if isinstance(values, FeatureBank):
        return values.features                               # (an fp8 bank raises TypeError: its rows are codes, not values)
    return values


def fill_missing(grid, values, seen, k=4, radius=None, weights="inverse", reach=None):
    """Give the rows feature fusion never saw the blend of their nearest seen neighbours.
    values fp16 / fp32 [N, C] over the grid's points (a heat-map, a fused feature matrix, or an fp16 FeatureBank); seen bool
    [N]: FeatureFusion.finish()'s point_ids as a mask, io.load_fused_features' mask_full.
    -> (filled [N, C], missing bool [N]): the seen rows bit for bit, every other row the blend of its (at most k) seen
    neighbours within `radius`; missing marks the unseen rows that found none (they keep 0).

    reach (cells): holes wider than a voxel.  The first stage is today's search -- at `radius` where that is at most
    voxel_size, else at voxel_size -- so the seen rows and the rows it fills are bit for bit what they are without `reach`.
    The rows it leaves go through PointIndex's second stage at `radius` (default and at most (reach + 1) * voxel_size): the
    blend of the seen points around the nearest voxel that holds one within `reach` cells -- the nearest of a stated
    candidate set, not the exact metric nearest neighbours.  missing then marks only the rows without a seen point within
    reach."""
    if not isinstance(grid, VoxelGrid):
        raise TypeError("grid must be a VoxelGrid")
    values = _values_of(values)
    if not isinstance(seen, torch.Tensor) or seen.dtype != torch.bool:
        raise TypeError("seen must be a bool tensor")
    if tuple(seen.shape) != (grid.n_points,) or seen.device != grid.device:
        raise ValueError("seen must be a bool [%d] mask on the grid's device" % grid.n_points)
    index = PointIndex(grid, sources=seen)
    if reach is None:
        nb = index.knn_self(k, radius=radius)
    else:
        wide = _radius(radius, grid.voxel_size, reach)
        nb = index.knn_self(k, radius=None if radius is None or float(radius) > grid.voxel_size else radius)
        nb = index._stage2(nb, grid.xyz, grid.coords, grid.inverse, None, ops.knn_k(k), wide, reach)
    blended, found = nb.blend(values, weights=weights, fill=0)
    return torch.where(seen[:, None], values, blended), ~(seen | found)


def smooth(grid, heat, k=8, radius=None):
    """The mean of every point's heat row over its k nearest points, itself included (uniform weights): what to threshold
    instead of the raw column when one stray point must not be one object.  heat fp16 / fp32 [N, Q] -> [N, Q]."""
    if not isinstance(grid, VoxelGrid):
        raise TypeError("grid must be a VoxelGrid")
    return PointIndex(grid).knn_self(k, radius=radius, include_self=True).blend(heat, weights="uniform")[0]
