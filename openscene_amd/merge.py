"""Merge regions by mean feature: the second stage after `openscene_amd.regions`.

A region of `segment` is a connected component of single linkage: a chain of pairwise similar voxels joins its two ends
however different they are.  A low threshold lets a wall leak into the door frame, a high one cuts every object into
fragments -- and `RegionResult.descriptors`, `.label` and `.point_labels` score a region by its mean feature, which means
something only for the right point set.  The usual answer: over-segment with a strict threshold, then merge ADJACENT regions
whose MEAN features agree.  The mean of a grown region does not drift along a chain.

    region_adjacency   which regions touch: the sorted distinct pairs (lo < hi) with their contact counts
    merge_regions      rounds of star contraction until nothing merges -> MergedRegions
    MergedRegions      a RegionResult (.regions, .groups, .descriptors, .label, .point_labels unchanged) plus
                       .parent (input region -> output region), .rounds, .converged, .history

A round (the contract is stated once, in include/openscene_amd.h): the unit rows of the regions' float32 sums; the fp32 dot
product of every adjacent pair with at least `min_contact` contacts; every region names its best eligible neighbour --
greatest similarity, then lowest pair index; a region is united with its best neighbour iff the two name each other (a
mutual pair) or the neighbour's own best pair is mutual.  A mutual pair plus the regions pointing at it is a star.  Mutual
pairs alone need one round per member of a blob, because the growing region becomes everybody's best neighbour; whole
best-neighbour trees are single linkage again.  What is exact: the similarities are fp32 sums in a fixed order; the best
neighbour is an integer maximum; the unions give the smallest member whatever the scheduling; the sums of the merged groups
are added row after row in ascending region id.  Two calls give identical tensors, and the regions stay numbered in ascending
order of their smallest voxel row.

Kernels: csrc/merge.hip through ops.regions_contacts / ops.rows_pair_dot / ops.regions_merge_round / ops.rows_fold, and
csrc/pool.hip for the regions' sums; no CPU path.  The unit rows, the numbering and the contraction of the pair list between
rounds (torch.unique and integer adds) are a few torch calls; the group count is read back once per round.
"""
import torch

from . import ops
from .objects import VoxelGrid
from .regions import RegionResult
from .search import FeatureBank


def region_adjacency(grid, voxel_region, n_regions, err=None):
    """Which regions touch.  voxel_region int32 [V] with values in -1 .. n_regions - 1 over the voxels of `grid`.
    -> (lo int32 [E], hi int32 [E], contacts int64 [E]): the distinct pairs lo < hi in ascending (lo, hi) order, and the number
    of neighbouring voxel pairs (the grid's connectivity, every undirected pair once) that realise each.  Voxels of region
    -1 touch nothing; scenes never touch.  The contact kernel runs once; compaction and counting are torch.unique."""
    if not isinstance(grid, VoxelGrid):
        raise TypeError("grid must be a VoxelGrid")
    if not isinstance(voxel_region, torch.Tensor) or voxel_region.dtype != torch.int32:
        raise TypeError("voxel_region must be an int32 tensor")
    if voxel_region.dim() != 1 or voxel_region.shape[0] != grid.n_voxels:
        raise ValueError("voxel_region holds %s entries, the grid %d voxels" % (tuple(voxel_region.shape), grid.n_voxels))
    if voxel_region.device != grid.device:
        raise ValueError("voxel_region and the grid must be on one device (%s, %s)" % (voxel_region.device, grid.device))
    key = ops.regions_contacts(voxel_region.contiguous(), grid.nbr, grid.connectivity, n_regions, err=err)
    pairs, contacts = torch.unique(key[key >= 0], return_counts=True)          # (sorted: ascending lo, then hi)
    return (pairs >> 32).to(torch.int32), (pairs & 0xFFFFFFFF).to(torch.int32), contacts


class MergedRegions(RegionResult):
    """A RegionResult after `merge_regions`, with
        parent      int64 [R_in]: the output region of every input region
        rounds      the rounds that merged something
        converged   True iff the last round merged nothing (or no pair was left): the partition is final for these arguments
        history     per executed round a dict: regions (before the round), pairs (with enough contacts), merged (regions lost)"""

    def __init__(self, names, offsets, voxel_size, n_regions, point_region, voxel_region, records, n_dropped_points, parent,
                 rounds, converged, history):
        super().__init__(names, offsets, voxel_size, n_regions, point_region, voxel_region, records, n_dropped_points)
        self.parent = parent
        self.rounds = int(rounds)
        self.converged = bool(converged)
        self.history = list(history)


def unit_rows(total):
    """fp16 [R, d]: the rows of the float32 sums `total` L2-normalised, zero rows left zero (the formula of Descriptors.queries)."""
    n = total.norm(dim=-1, keepdim=True)
    return torch.where(n > 0, total / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(total)).half()


def merge_regions(bank, grid, regions, similarity=0.8, min_contact=1, max_rounds=64):
    """Merge the adjacent regions of `regions` (a RegionResult of `grid` over `bank`) whose mean features agree.

    similarity   two regions may merge when the fp32 dot product of their unit mean rows is >= similarity (finite)
    min_contact  ... and at least this many neighbouring voxel pairs join them (>= 1); contacts add up as regions merge
    max_rounds   at most this many rounds (>= 0); `converged` tells whether the loop ended by itself
    0.8 and 64 are interface defaults, not tuned values.  Zero regions, or no adjacent regions, returns the input partition
    with rounds == 0.  Regions dropped by `min_points` (-1) stay dropped.  The records come from ops.regions_records on the new
    labelling; names, offsets and n_dropped_points are carried over.  One read-back per round.  -> MergedRegions"""
    if not isinstance(bank, FeatureBank):
        raise TypeError("bank must be a FeatureBank")
    if not isinstance(grid, VoxelGrid):
        raise TypeError("grid must be a VoxelGrid")
    if not isinstance(regions, RegionResult):
        raise TypeError("regions must be a RegionResult")
    if bank.rows != grid.n_points:
        raise ValueError("the bank holds %d rows, the grid %d points: they must describe the same points" % (bank.rows, grid.n_points))
    if bank.device != grid.device or regions.voxel_region.device != grid.device:
        raise ValueError("the bank, the grid and the regions must be on one device (%s, %s, %s)"
                         % (bank.device, grid.device, regions.voxel_region.device))
    if regions.voxel_region.shape[0] != grid.n_voxels or regions.point_region.shape[0] != grid.n_points:
        raise ValueError("the regions label %d voxels and %d points, the grid has %d and %d"
                         % (regions.voxel_region.shape[0], regions.point_region.shape[0], grid.n_voxels, grid.n_points))
    if bank.dim > ops.BANK_POOL_MAX_DIM:
        raise ValueError("rows of up to %d features can be merged (the bank has %d)" % (ops.BANK_POOL_MAX_DIM, bank.dim))
    similarity = float(similarity)
    if similarity != similarity or similarity in (float("inf"), float("-inf")):
        raise ValueError("similarity must be finite (got %r)" % (similarity,))
    min_contact = int(min_contact)
    if min_contact < 1:
        raise ValueError("min_contact must be at least 1 (got %d)" % min_contact)
    max_rounds = int(max_rounds)
    if max_rounds < 0:
        raise ValueError("max_rounds must not be negative (got %d)" % max_rounds)
    dev = grid.device
    r = regions.n_regions
    parent = torch.arange(r, dtype=torch.int64, device=dev)
    history, rounds, converged = [], 0, True
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    if r > 0:
        lo, hi, contacts = region_adjacency(grid, regions.voxel_region, r, err=err)
        ops.regions_check(err)
        converged = lo.shape[0] == 0
        total = regions.descriptors(bank).sum if lo.shape[0] else None
        for _ in range(max_rounds if lo.shape[0] else 0):
            enough = contacts >= min_contact
            elo, ehi = lo[enough].contiguous(), hi[enough].contiguous()
            if elo.shape[0] == 0:
                converged = True
                break
            sim = ops.rows_pair_dot(unit_rows(total), elo, ehi, err=err)
            root = ops.regions_merge_round(elo, ehi, sim, r, similarity, err=err).long()
            # number the groups in ascending order of their smallest member: mark, cumulative sum, select
            number = torch.cumsum(root == torch.arange(r, device=dev), 0) - 1
            new_id = number[root]
            g, bits = torch.cat([number[-1:] + 1, err.long()]).tolist()         # the read-back of the round
            if bits:
                ops.regions_check(err)
            history.append({"regions": r, "pairs": int(elo.shape[0]), "merged": r - g})
            if g == r:
                converged = True
                break
            rounds += 1
            converged = False
            # the sums of the groups: members in ascending old id
            members = torch.sort(new_id, stable=True)[1].to(torch.int32)
            starts = torch.zeros(g + 1, dtype=torch.int64, device=dev)
            starts[1:] = torch.cumsum(torch.bincount(new_id, minlength=g), 0)
            total = ops.rows_fold(total, starts, members, err=err)
            # contract the pair list: map both ends, drop equal ends, restore lo < hi, add the contacts of equal pairs
            a, b = new_id[lo.long()], new_id[hi.long()]
            apart = a != b
            a, b, c = a[apart], b[apart], contacts[apart]
            pairs, inverse = torch.unique(torch.minimum(a, b) * g + torch.maximum(a, b), return_inverse=True)
            contacts = torch.zeros(pairs.shape[0], dtype=torch.int64, device=dev).index_add_(0, inverse, c)
            lo, hi = torch.div(pairs, g, rounding_mode="floor").to(torch.int32), (pairs % g).to(torch.int32)
            parent = new_id[parent]
            r = g
            if lo.shape[0] == 0:
                converged = True
                break
        ops.regions_check(err)
    old = regions.voxel_region.long()
    voxel_region = torch.where(old >= 0, parent[old.clamp(min=0)] if parent.numel() else old, old).to(torch.int32)
    rec = ops.regions_records(voxel_region, r, grid.xyz, grid.inverse, grid.coords, err=err)
    point_region = voxel_region[grid.inverse.long()]
    ops.regions_check(err)
    return MergedRegions(regions.names, regions.offsets, regions.voxel_size, r, point_region, voxel_region, rec,
                         regions.n_dropped_points, parent, rounds, converged, history)
