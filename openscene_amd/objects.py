"""Find objects in heat-maps: the reference README's "Applications" -- rare object search in a scene database,
image-based 3-D object detection, interactive object search -- want to know WHERE in a scene the matches are, how many
there are, how large each one is and how confident the match is.  `openscene_amd.search` gives the heat-map; here:

    VoxelGrid        built once for a set of scenes: voxel rows, point -> voxel map, 3^3 neighbour table
    find_objects     heat-map [N, Q] + thresholds -> per (scene, query) the best M objects, ranked
    ObjectResult     .objects(scene, q) as plain dicts, .rank_scenes(q, by=...), .descriptors(bank) (an object as the next query)

An object is a connected component (26- or 6-neighbourhood) of the voxels that hold at least one hit -- a point whose score
is finite and >= the query's threshold.  Every field is an integer, a selected input value, or derived on the host from
exact integers: results are exact and bitwise repeatable.

Kernels: csrc/objects.hip through ops.objects_find; no CPU path.
"""
import torch

from . import ops

COORD_LIMIT = 32767          # |voxel coordinate| < this (the packable range of ops.coords_unique)
SCENE_LIMIT = 65535


class VoxelGrid:
    """The voxels of a set of scenes: ``floor(xyz.double() / voxel_size)`` as int32 with the scene index as the batch column.

    xyz float [N, 3] on the device; offsets: the bank's S + 1 row offsets (None = one scene).  Holds
        xyz       float32 [N, 3] (the boxes are taken over these)
        coords    int32 [V, 4] unique (scene, x, y, z) rows       inverse  int32 [N] point -> voxel row
        nbr       int32 [27, V] neighbour table of the rows over themselves
        table     the hash table of the rows (ops.HashTable; None for an empty grid): what ops.kmap_build probes for foreign cells
    Points of different scenes never share or neighbour a voxel.  A coordinate outside the packable range raises."""

    def __init__(self, xyz, offsets=None, voxel_size=0.05, connectivity=26):
        if connectivity not in (6, 26):
            raise ValueError("connectivity must be 6 or 26 (got %r)" % (connectivity,))
        voxel_size = float(voxel_size)
        if not voxel_size > 0:
            raise ValueError("voxel_size must be positive (got %r)" % voxel_size)
        if not isinstance(xyz, torch.Tensor) or not xyz.dtype.is_floating_point or xyz.dim() != 2 or xyz.shape[1] != 3:
            raise TypeError("xyz must be a float [N, 3] tensor")
        n = xyz.shape[0]
        if n >= ops.OBJECTS_MAX_POINTS:
            raise ValueError("at most 2^22 - 1 points per grid (got %d)" % n)
        offsets = [0, n] if offsets is None else [int(o) for o in (offsets.tolist() if isinstance(offsets, torch.Tensor) else offsets)]
        if len(offsets) < 1 or offsets[0] != 0 or offsets[-1] != n or any(b < a for a, b in zip(offsets[:-1], offsets[1:])):
            raise ValueError("offsets must ascend from 0 to the number of points (%d)" % n)
        if len(offsets) - 1 >= SCENE_LIMIT:
            raise ValueError("fewer than %d scenes per grid (got %d)" % (SCENE_LIMIT, len(offsets) - 1))
        dev = xyz.device
        self.device = dev
        self.voxel_size = voxel_size
        self.connectivity = connectivity
        self.offsets = offsets
        self.xyz = xyz.detach().float().contiguous()
        self._offsets_dev = torch.tensor(offsets, dtype=torch.int64).to(dev)
        if n == 0:
            self.coords = torch.empty((0, 4), dtype=torch.int32, device=dev)
            self.inverse = torch.empty(0, dtype=torch.int32, device=dev)
            self.nbr = torch.empty((27, 0), dtype=torch.int32, device=dev)
            self.table = None
            return
        cell = torch.floor(xyz.detach().double() / voxel_size)
        if not bool(((cell > -COORD_LIMIT) & (cell < COORD_LIMIT)).all()):          # (NaN and inf fail it too)
            raise ValueError("a voxel coordinate outside the packable range: |floor(xyz / voxel_size)| must stay below %d"
                             % COORD_LIMIT)
        rows = torch.tensor([b - a for a, b in zip(offsets[:-1], offsets[1:])], dtype=torch.int64).to(dev)
        scene = torch.repeat_interleave(torch.arange(len(offsets) - 1, device=dev), rows, output_size=n)
        coords4 = torch.cat([scene.to(torch.int32)[:, None], cell.to(torch.int32)], 1).contiguous()
        self.coords, self.inverse, _first, self.table = ops.coords_unique(coords4)
        self.coords = self.coords.contiguous()
        self.inverse = self.inverse.contiguous()
        self.nbr = ops.kmap_build(self.table, self.coords, 3, 1, self_map=True)

    @classmethod
    def from_scenes(cls, scenes, voxel_size=0.05, connectivity=26):
        """One grid over a list of per-scene xyz tensors, in list order."""
        scenes = list(scenes)
        if not scenes:
            raise ValueError("no scene given")
        offsets = [0]
        for x in scenes:
            offsets.append(offsets[-1] + x.shape[0])
        return cls(torch.cat(scenes, 0), offsets, voxel_size, connectivity)

    @property
    def n_points(self):
        return self.xyz.shape[0]

    @property
    def n_voxels(self):
        return self.coords.shape[0]

    @property
    def n_scenes(self):
        return len(self.offsets) - 1

    def offsets_tensor(self):
        """int64 [S + 1] on the device."""
        return self._offsets_dev


FIELDS = ("n_points", "n_voxels", "peak_score", "peak_point", "score_sum", "vox_sum", "box_min", "box_max")


class ObjectResult:
    """Per (scene, query) the kept objects, best first, as [S, Q, M] tensors:
        n_points, n_voxels int64; peak_score fp16 (the maximum score); peak_point int64 (the lowest row inside its scene that
        attains it); score_sum int64 (sum of score * 2**24, exact); vox_sum int64 [.., 3]; box_min / box_max float32 [.., 3]
        mean_score = score_sum.double() / 2**24 / n_points and centroid = (vox_sum.double() / n_points + 0.5) * voxel_size,
        float64, formed from the exact integers (NaN in padding slots)
    n_objects int64 [S, Q]: the objects that passed `min_points`, before the cap.  Padding slots: n_points 0, peak_point -1,
    peak_score -inf.  point_object int32 [N, Q] or None: the rank of the kept object a hit belongs to, else -1."""

    def __init__(self, names, offsets, voxel_size, fields, n_objects, point_object):
        self.names = list(names)
        self.offsets = list(offsets)
        self.voxel_size = float(voxel_size)
        for f in FIELDS:
            setattr(self, f, fields[f])
        self.n_objects = n_objects
        self.point_object = point_object
        cnt = self.n_points.double()
        self.mean_score = self.score_sum.double() / 2 ** 24 / cnt
        self.centroid = (self.vox_sum.double() / cnt[..., None] + 0.5) * self.voxel_size

    def _scene(self, which):
        return self.names.index(which) if isinstance(which, str) else int(which)

    def _query(self, q):
        q = int(q)
        if not 0 <= q < self.n_points.shape[1]:
            raise IndexError("query %d of %d" % (q, self.n_points.shape[1]))
        return q

    def objects(self, scene, q):
        """The kept objects of one scene (name or position) for query `q`, best first, as plain dicts."""
        s, q = self._scene(scene), self._query(q)
        kept = int((self.n_points[s, q] > 0).sum())
        cols = {f: getattr(self, f)[s, q, :kept].cpu() for f in FIELDS + ("mean_score", "centroid")}
        out = []
        for i in range(kept):
            out.append({"rank": i, "n_points": int(cols["n_points"][i]), "n_voxels": int(cols["n_voxels"][i]),
                        "peak_score": float(cols["peak_score"][i]), "peak_point": int(cols["peak_point"][i]),
                        "mean_score": float(cols["mean_score"][i]), "centroid": cols["centroid"][i].tolist(),
                        "box_min": cols["box_min"][i].tolist(), "box_max": cols["box_max"][i].tolist()})
        return out

    def rank_scenes(self, q, by="objects"):
        """[(scene name, value)] for query `q`, best first, ties in scene order.  by = "objects": the number of objects that
        passed the filter; "peak": the best object's peak score; "largest": the points of the largest kept object.  A scene
        without objects scores 0 (-inf for "peak")."""
        q = self._query(q)
        if by == "objects":
            score = self.n_objects[:, q].double()
        elif by == "peak":
            score = self.peak_score[:, q, 0].double()
        elif by == "largest":
            score = self.n_points[:, q, :].max(1)[0].double()
        else:
            raise ValueError('by must be "objects", "peak" or "largest" (got %r)' % (by,))
        score = score.cpu()
        order = torch.sort(score, descending=True, stable=True)[1].tolist()
        vals = score.tolist()
        return [(self.names[i], vals[i] if by == "peak" else int(vals[i])) for i in order]

    def descriptors(self, bank, heat=None):
        """Descriptors [S, Q, M] of the kept objects over `bank`, the bank whose heat-map was searched
        (openscene_amd.descriptors.describe_objects): the mean normalised feature row of every object's hits, with `heat`
        weighted by max(score, 0).  Needs find_objects(..., return_point_ids=True)."""
        from .descriptors import describe_objects
        return describe_objects(self, bank, heat)


def find_objects(grid, heat, thresholds, min_points=1, max_objects=16, return_point_ids=False, names=None):
    """Objects of every (scene, query) of a heat-map over the grid's points.

    heat fp16 [N, Q]: what ``search(..., return_heat=True).heat`` or ``heat_map`` returns for the grid's points.
    thresholds: a number or Q numbers.  Objects of fewer than `min_points` hits are dropped; the rest are ordered by peak
    score, then peak point, and the first `max_objects` (1 .. 64) kept.  The number of components is read back from the
    device once per call (one synchronisation).  -> ObjectResult."""
    if not isinstance(grid, VoxelGrid):
        raise TypeError("grid must be a VoxelGrid")
    if not isinstance(heat, torch.Tensor) or heat.dtype != torch.float16:
        raise TypeError("heat must be a float16 tensor (got %s)" % (heat.dtype if isinstance(heat, torch.Tensor) else type(heat).__name__))
    if heat.dim() != 2 or heat.shape[0] != grid.n_points or heat.shape[1] < 1:
        raise ValueError("heat must be [%d, Q] for this grid (got %s)" % (grid.n_points, tuple(heat.shape)))
    if heat.device != grid.device:
        raise ValueError("heat must be on the grid's device (%s, got %s)" % (grid.device, heat.device))
    if heat.shape[0] >= ops.OBJECTS_MAX_POINTS:
        raise ValueError("at most 2^22 - 1 points per call (got %d)" % heat.shape[0])
    q = heat.shape[1]
    max_objects, min_points = int(max_objects), int(min_points)
    if not 1 <= max_objects <= ops.OBJECTS_MAX_M:
        raise ValueError("max_objects must be in 1 .. %d (got %d)" % (ops.OBJECTS_MAX_M, max_objects))
    if min_points < 1:
        raise ValueError("min_points must be at least 1 (got %d)" % min_points)
    thresholds = torch.as_tensor(thresholds, dtype=torch.float32).reshape(-1)
    if thresholds.numel() == 1 and q > 1:
        thresholds = thresholds.expand(q)
    if thresholds.numel() != q:
        raise ValueError("%d thresholds for %d queries" % (thresholds.numel(), q))
    thresholds = thresholds.contiguous().to(grid.device)
    if names is None:
        names = [str(i) for i in range(grid.n_scenes)]
    elif len(names) != grid.n_scenes:
        raise ValueError("%d names for %d scenes" % (len(names), grid.n_scenes))
    out = ops.objects_find(heat.contiguous(), thresholds, grid.xyz, grid.inverse, grid.coords, grid.nbr, grid.offsets_tensor(),
                           connectivity=grid.connectivity, min_points=min_points, max_objects=max_objects,
                           return_point_ids=bool(return_point_ids))
    return ObjectResult(names, grid.offsets, grid.voxel_size, out, out["n_objects"], out["point_object"])
