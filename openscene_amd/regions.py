"""Segment scenes without a prompt: the reference README's first application -- "open-vocabulary 3D scene understanding
and exploration" (materials, affordances, room type, "what is in this room?") -- wants a partition of a scene that exists
before anyone has typed a word and serves every later prompt.  `find_objects` cuts a scene where a heat-map is over a
threshold; here the grouping rule needs no heat-map: two neighbouring voxels belong together when their features agree.

    SimilarityGraph   built once per bank and grid: one unit feature row per voxel and the dot product of every pair of
                      neighbouring voxels
    graph.segment     threshold the edges, connected components, exact records -> RegionResult (cheap: move the threshold
                      interactively, the dot products are not redone)
    segment           the one-call form
    RegionResult      .regions(scene) as plain dicts, .groups() / .descriptors(bank) (a region as the next query),
                      .label(bank, text_features) (label every region with a vocabulary), .point_labels(classes)

A region is a connected component of SINGLE LINKAGE over neighbouring voxels (26 or 6 neighbours, the grid's): a chain of
pairwise similar voxels joins its two ends however different they are (`openscene_amd.merge` is the second stage for
that: cut strictly here, then merge adjacent regions by their mean features).  What is exact: the partition is the connected
components of the graph of edges whose float32 similarity is >= the threshold -- a property of the similarities, not of
scheduling --, the numbering is canonical (regions in ascending order of their smallest voxel row), and every record
field is an integer, a selected input value, or derived on the host from exact integers.  The similarities themselves
are fp32 sums in a fixed order: bitwise repeatable.

Kernels: csrc/regions.hip through ops.regions_edges / ops.regions_label / ops.regions_records, csrc/pool.hip for the voxel
rows; no CPU path.  Numbering the roots and the `min_points` filter are a few torch calls.
"""
import torch

from . import ops
from .descriptors import PointGroups, pool
from .objects import VoxelGrid
from .search import FeatureBank, heat_map

SLICE_VOXELS = 1 << 15       # voxel rows pooled per call: bounds the float32 temporaries at a few times SLICE_VOXELS * dim * 4 bytes

FIELDS = ("scene", "n_points", "n_voxels", "vox_sum", "box_min", "box_max")


def voxel_rows(bank, grid, slice_voxels=SLICE_VOXELS):
    """(vox fp16 [V, D], points per voxel int64 [V]): ``pool(bank, PointGroups.from_labels(grid.inverse, V)).queries()`` built in
    slices of `slice_voxels` voxels.  The CSR form from_labels builds (rows ascending inside a voxel) is made once and cut;
    a group's bits do not depend on its place in the list (`pool`), so the slices change no bit."""
    v = grid.n_voxels
    inv = grid.inverse.long()
    order = torch.sort(inv, stable=True)[1]
    starts = torch.zeros(v + 1, dtype=torch.int64, device=grid.device)
    if v:
        starts[1:] = torch.cumsum(torch.bincount(inv, minlength=v), 0)
    cuts = starts[::slice_voxels].tolist() + [grid.n_points]          # (one read-back for all the slices)
    vox = torch.empty((v, bank.dim), dtype=torch.float16, device=grid.device)
    for i, a in enumerate(range(0, v, slice_voxels)):
        b = min(a + slice_voxels, v)
        groups = PointGroups(starts[a:b + 1] - cuts[i], order[cuts[i]:cuts[i + 1]], (b - a,), _checked=True)
        vox[a:b] = pool(bank, groups).queries()
    return vox, starts[1:] - starts[:-1]


class SimilarityGraph:
    """The voxels of `grid` with one feature row each and the similarity of every pair of neighbouring voxels.

    vox   fp16 [V, D]: ``pool(bank, PointGroups.from_labels(grid.inverse, V)).queries()`` -- the L2-normalised mean of the
          normalised rows of the voxel's points, for either bank kind (an fp8 bank is never dequantised)
    sim   float32 [n_off, V]: ``ops.regions_edges(vox, grid.nbr, grid.connectivity)``; n_off = 13 (connectivity 26) or 3
    The rows are built in slices of `slice_voxels` voxels so the float32 temporaries stay bounded.  `pool` guarantees that
    a group's bits do not depend on its place in the list, so slicing changes no bit of `vox`.
    bank.rows must equal grid.n_points (row i of the bank is point i of the grid) and the devices must match."""

    def __init__(self, bank, grid, slice_voxels=SLICE_VOXELS):
        if not isinstance(bank, FeatureBank):
            raise TypeError("bank must be a FeatureBank")
        if not isinstance(grid, VoxelGrid):
            raise TypeError("grid must be a VoxelGrid")
        if bank.rows != grid.n_points:
            raise ValueError("the bank holds %d rows, the grid %d points: they must describe the same points" % (bank.rows, grid.n_points))
        if bank.device != grid.device:
            raise ValueError("the bank and the grid must be on one device (%s, %s)" % (bank.device, grid.device))
        if bank.dim > ops.BANK_POOL_MAX_DIM:
            raise ValueError("rows of up to %d features can be segmented (the bank has %d)" % (ops.BANK_POOL_MAX_DIM, bank.dim))
        slice_voxels = int(slice_voxels)
        if slice_voxels < 1:
            raise ValueError("slice_voxels must be at least 1 (got %d)" % slice_voxels)
        self.grid = grid
        self.dim = bank.dim
        self.vox, self.points_per_voxel = voxel_rows(bank, grid, slice_voxels)
        self.sim = ops.regions_edges(self.vox, grid.nbr, grid.connectivity)

    def segment(self, similarity=0.9, min_points=1, names=None):
        """Regions at one threshold: neighbouring voxels with sim >= `similarity` (float32) are joined, regions of fewer
        than `min_points` points are dropped.  Runs the label and record kernels only -- `sim` is reused as it is.
        similarity must be finite; the default 0.9 is an interface default, not a tuned value.  The number of regions is
        read back from the device once per call, to size the records; the err word is read once more at the end.
        -> RegionResult."""
        similarity = float(similarity)
        if similarity != similarity or similarity in (float("inf"), float("-inf")):
            raise ValueError("similarity must be finite (got %r)" % (similarity,))
        min_points = int(min_points)
        if min_points < 1:
            raise ValueError("min_points must be at least 1 (got %d)" % min_points)
        grid = self.grid
        if names is None:
            names = [str(i) for i in range(grid.n_scenes)]
        elif len(names) != grid.n_scenes:
            raise ValueError("%d names for %d scenes" % (len(names), grid.n_scenes))
        dev = grid.device
        v = grid.n_voxels
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        root = ops.regions_label(self.sim, grid.nbr, grid.connectivity, similarity, err=err)
        # number the kept roots in ascending row order: mark, cumulative sum, select
        rl = root.long()
        points = torch.zeros(v, dtype=torch.int64, device=dev).index_add_(0, rl, self.points_per_voxel)
        keep = (rl == torch.arange(v, device=dev)) & (points >= min_points)
        number = torch.cumsum(keep, 0) - 1
        voxel_region = torch.where(keep[rl], number[rl], torch.full_like(rl, -1)).to(torch.int32)
        count = number[-1:] + 1 if v else torch.zeros(1, dtype=torch.int64, device=dev)
        kept_points = (points * keep).sum().reshape(1)
        n_regions, bits, kept_points = torch.cat([count, err.long(), kept_points]).tolist()      # the read-back of R
        if bits:
            ops.regions_check(err)
        rec = ops.regions_records(voxel_region, n_regions, grid.xyz, grid.inverse, grid.coords, err=err)
        point_region = voxel_region[grid.inverse.long()]
        ops.regions_check(err)                                             # (the records' own skips; the arrays are the grid's)
        return RegionResult(names, grid.offsets, grid.voxel_size, n_regions, point_region, voxel_region, rec,
                            grid.n_points - kept_points)


def segment(bank, grid, similarity=0.9, min_points=1, names=None, slice_voxels=SLICE_VOXELS):
    """The regions of `grid`'s scenes by the features of `bank` in one call: ``SimilarityGraph(bank, grid).segment(...)``.
    names defaults to the bank's scene names when it has as many scenes as the grid."""
    graph = SimilarityGraph(bank, grid, slice_voxels)
    if names is None and len(bank.names) == grid.n_scenes:
        names = bank.names
    return graph.segment(similarity, min_points, names)


class RegionResult:
    """The regions of a set of scenes, numbered 0 .. R - 1 over the whole grid in ascending order of their smallest voxel row:
        n_regions      R
        point_region   int32 [N] (-1: the point's region was dropped by `min_points`)     voxel_region  int32 [V]
        scene int32, n_points, n_voxels int64 [R]; vox_sum int64 [R, 3]; box_min / box_max float32 [R, 3]
        centroid       float64 [R, 3] = (vox_sum / n_points + 0.5) * voxel_size, formed from the exact integers
        n_dropped_points   the points with point_region -1"""

    def __init__(self, names, offsets, voxel_size, n_regions, point_region, voxel_region, records, n_dropped_points):
        self.names = list(names)
        self.offsets = list(offsets)
        self.voxel_size = float(voxel_size)
        self.n_regions = int(n_regions)
        self.point_region = point_region
        self.voxel_region = voxel_region
        for f in FIELDS:
            setattr(self, f, records[f])
        self.centroid = (self.vox_sum.double() / self.n_points.double()[:, None] + 0.5) * self.voxel_size
        self.n_dropped_points = int(n_dropped_points)

    def _scene(self, which):
        return self.names.index(which) if isinstance(which, str) else int(which)

    def regions(self, scene):
        """The regions of one scene (name or position) as plain dicts, largest first, ties by id."""
        s = self._scene(scene)
        if not 0 <= s < len(self.names):
            raise IndexError("scene %d of %d" % (s, len(self.names)))
        ids = torch.nonzero(self.scene.cpu() == s).reshape(-1)
        cols = {f: getattr(self, f).cpu()[ids] for f in FIELDS[1:] + ("centroid",)}
        order = torch.sort(cols["n_points"], descending=True, stable=True)[1].tolist()
        return [{"id": int(ids[i]), "n_points": int(cols["n_points"][i]), "n_voxels": int(cols["n_voxels"][i]),
                 "centroid": cols["centroid"][i].tolist(), "box_min": cols["box_min"][i].tolist(),
                 "box_max": cols["box_max"][i].tolist()} for i in order]

    def groups(self):
        """The regions as point sets over the bank the grid's points are the rows of: ``PointGroups.from_labels``."""
        return PointGroups.from_labels(self.point_region, self.n_regions)

    def descriptors(self, bank):
        """Descriptors [R] of the regions over `bank` (openscene_amd.descriptors.pool): ``.queries()`` makes a region the
        next query of `search`."""
        return pool(bank, self.groups())

    def label(self, bank, text_features, negatives=None, temperature=0.1):
        """Label every region with a vocabulary: text_features fp16 [C, dim], L2-normalised (``util/util.py:41-44``).
        The scores are ``heat_map(descriptors(bank).mean, text_features, ...)`` -- the per-point scoring formula of `search`
        (relevancies when negatives are given) applied to the region's mean feature.
        -> (class int64 [R]: the lowest index among the maxima (ops.rows_argmax), score fp16 [R]: its score)."""
        dev = self.point_region.device
        if self.n_regions == 0:
            return torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.float16, device=dev)
        heat = heat_map(self.descriptors(bank).mean, text_features, negatives=negatives, temperature=temperature)
        classes = ops.rows_argmax(heat.float())
        return classes, heat.gather(1, classes[:, None])[:, 0]

    def point_labels(self, classes):
        """int64 [N]: every point gets its region's class, -1 where its region was dropped -- ready for the ids path of
        OpenVocabEvaluator."""
        if not isinstance(classes, torch.Tensor) or classes.dim() != 1 or classes.shape[0] != self.n_regions \
                or classes.dtype.is_floating_point:
            raise ValueError("classes must be a vector of %d integers, one per region" % self.n_regions)
        classes = classes.long().to(self.point_region.device)
        region = self.point_region.long()
        out = torch.full_like(region, -1)
        kept = region >= 0
        out[kept] = classes[region[kept]]
        return out
