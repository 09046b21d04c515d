"""Search a bank of scenes by text (or image) embedding: the reference README's "Applications" -- scene exploration by
free text, rare object search in a 3D scene database, image-based retrieval -- on per-point OpenScene features.

The reference forms the features (``run/evaluate.py:290`` distill, ``:285`` fusion, ``:318`` ensemble), scores them
against CLIP text embeddings (``:291``, ``:305,310``) and can save them per scene (``save_feature_as_numpy``,
``:232-235,328-330``: ``<scene>_openscene_feat_<feature_type>.npy``).  Here:

    FeatureBank      one growing fp16 matrix of per-point features, many scenes, on the device
    search           heat-map [N, Q] + the k best points of every scene + counts over a threshold: ONE pass over the bank
    heat_map         the one-scene convenience
    SearchResult     .rank_scenes(q, by=...) orders the scenes for a query; .find_objects(grid, thresholds) groups the
                     heat-map into ranked objects (openscene_amd.objects)

Kernels: csrc/search.hip through ops.bank_append / ops.bank_search; no CPU path.
"""
import numpy as np
import torch

from . import io as _io
from . import ops


class FeatureBank:
    """A growing fp16 [rows, dim] matrix on `device` holding the per-point features of many scenes back to back.

    offsets  python list, S + 1 ascending row offsets (scene i is rows offsets[i] : offsets[i + 1])
    names    python list of the S scene names (unique)
    """

    def __init__(self, dim, device, capacity_rows=1 << 16):
        dim = int(dim)
        if dim < 8 or dim % 8:
            raise ValueError("dim must be a positive multiple of 8 (got %d)" % dim)
        self.dim = dim
        self.device = torch.device(device)
        self._data = torch.empty((max(int(capacity_rows), 1), dim), dtype=torch.float16, device=self.device)
        self.offsets = [0]
        self.names = []
        self._offsets_dev = None
        self._err = None

    # ---- views
    def __len__(self):
        return len(self.names)

    @property
    def rows(self):
        return self.offsets[-1]

    @property
    def capacity_rows(self):
        return self._data.shape[0]

    @property
    def features(self):
        """fp16 [rows, dim]: a view of the filled part."""
        return self._data[:self.rows]

    def scene(self, which):
        """fp16 [n, dim] view of one scene's rows (by name or position)."""
        i = self.names.index(which) if isinstance(which, str) else int(which)
        return self._data[self.offsets[i]:self.offsets[i + 1]]

    def scene_rows(self):
        return [b - a for a, b in zip(self.offsets[:-1], self.offsets[1:])]

    def offsets_tensor(self):
        """int64 [S + 1] on the device (cached until the next scene is added)."""
        if self._offsets_dev is None:
            self._offsets_dev = torch.tensor(self.offsets, dtype=torch.int64).to(self.device)
        return self._offsets_dev

    def _err_word(self):
        if self._err is None:
            self._err = torch.zeros(1, dtype=torch.int32, device=self.device)
        return self._err

    # ---- growth
    def _reserve(self, n):
        need = self.rows + n
        if need <= self._data.shape[0]:
            return
        cap = max(need, 2 * self._data.shape[0])
        data = torch.empty((cap, self.dim), dtype=torch.float16, device=self.device)
        data[:self.rows].copy_(self._data[:self.rows])
        self._data = data

    def _commit(self, name, n):
        self.offsets.append(self.rows + n)
        self.names.append(name)
        self._offsets_dev = None

    def add_scene(self, name, features, inds_reverse=None):
        """Append one scene.  float32 features on the bank's device -- the network output, with the voxel -> point
        map `inds_reverse`: exactly ``predictions = feat_3d[inds_reverse]`` of ``run/evaluate.py:290``, stored as the
        ``.half()`` of ``:291`` -- go through the fused gather + cast kernel; fp16 features (fused / ensemble features,
        saved files) are copied as they are.  An index outside the feature matrix raises and leaves the bank as it
        was.  -> the scene's position."""
        name = str(name)
        if name in self.names:
            raise ValueError("the bank already holds a scene named %r" % name)
        if isinstance(features, np.ndarray):
            features = torch.from_numpy(features)
        if features.dim() != 2 or features.shape[1] != self.dim:
            raise ValueError("features must be [points, %d] (got %s)" % (self.dim, tuple(features.shape)))
        if features.dtype == torch.float16:
            rows = features if inds_reverse is None else features[torch.as_tensor(inds_reverse).long().to(features.device)]
            n = rows.shape[0]
            self._reserve(n)
            self._data[self.rows:self.rows + n].copy_(rows)
        elif features.dtype == torch.float32:
            features = features.to(self.device)
            if inds_reverse is not None:
                inds_reverse = torch.as_tensor(inds_reverse).to(self.device)
                if inds_reverse.dim() != 1 or inds_reverse.dtype.is_floating_point or inds_reverse.dtype == torch.bool:
                    raise TypeError("inds_reverse must be a vector of integer indices")
            n = features.shape[0] if inds_reverse is None else inds_reverse.shape[0]
            self._reserve(n)
            err = self._err_word()
            ops.bank_append(self._data, self.rows, features, err, gather=inds_reverse)
            try:
                ops.bank_check(err)
            except Exception:
                err.zero_()                       # rows past `rows` are scratch: the bank is as it was
                raise
        else:
            raise TypeError("features must be float32 or float16 (got %s)" % features.dtype)
        self._commit(name, n)
        return len(self.names) - 1

    def add_saved(self, folder, feature_type):
        """Append every ``<scene>_openscene_feat_<feature_type>.npy`` of `folder` (``run/evaluate.py:328-330``; float32 or
        float16 arrays), in file-name order; the scene name is the part before the tag.  -> the names added."""
        added = []
        for name, path in _io.list_point_features(folder, feature_type):
            arr = np.load(path)
            if arr.dtype not in (np.float32, np.float16):
                raise TypeError("%s holds %s features (float32 or float16 expected)" % (path, arr.dtype))
            self.add_scene(name, torch.from_numpy(arr))
            added.append(name)
        return added

    # ---- persistence
    def save(self, path):
        """One file: the filled rows (fp16), the offsets and the names."""
        torch.save({"dim": self.dim, "offsets": list(self.offsets), "names": list(self.names),
                    "features": self.features.cpu().clone()}, path)

    @classmethod
    def load(cls, path, device):
        d = torch.load(path, map_location="cpu", weights_only=False)
        feats = d["features"]
        if feats.dtype != torch.float16 or feats.dim() != 2 or feats.shape[1] != d["dim"] or feats.shape[0] != d["offsets"][-1]:
            raise ValueError("%s is not a feature bank" % path)
        bank = cls(d["dim"], device, capacity_rows=max(feats.shape[0], 1))
        bank._data[:feats.shape[0]].copy_(feats)
        bank.offsets = [int(o) for o in d["offsets"]]
        bank.names = [str(n) for n in d["names"]]
        return bank


class SearchResult:
    """topk_scores fp16 [S, Q, k], topk_points int64 [S, Q, k] (row inside its scene; -1 with score -inf pads a scene
    of fewer than k points), counts int64 [S, Q] or None (points with score >= the query's threshold), heat fp16 [N, Q]
    or None, names (the bank's scene names), offsets."""

    def __init__(self, names, offsets, topk_scores, topk_points, counts, heat):
        self.names = list(names)
        self.offsets = list(offsets)
        self.topk_scores = topk_scores
        self.topk_points = topk_points
        self.counts = counts
        self.heat = heat

    def scene_heat(self, which):
        """fp16 [n, Q] view of one scene's rows of the heat-map."""
        if self.heat is None:
            raise ValueError("the search was run without return_heat")
        i = self.names.index(which) if isinstance(which, str) else int(which)
        return self.heat[self.offsets[i]:self.offsets[i + 1]]

    def rank_scenes(self, q, by="max"):
        """[(scene name, score)] for query `q`, best first, ties in scene order.  by = "max": the best point's score;
        "topk_mean": the mean of the (up to k) selected scores; "count": the points over the threshold.  A scene
        without points scores -inf (0 for "count")."""
        q = int(q)
        if not 0 <= q < self.topk_scores.shape[1]:
            raise IndexError("query %d of %d" % (q, self.topk_scores.shape[1]))
        if by == "max":
            score = self.topk_scores[:, q, 0].float()
        elif by == "topk_mean":
            s = self.topk_scores[:, q, :].float()
            valid = self.topk_points[:, q, :] >= 0
            cnt = valid.sum(1)
            score = torch.where(valid, s, torch.zeros_like(s)).sum(1) / cnt.clamp(min=1)
            score = torch.where(cnt > 0, score, torch.full_like(score, float("-inf")))
        elif by == "count":
            if self.counts is None:
                raise ValueError('by="count" needs a search with thresholds')
            score = self.counts[:, q].double()
        else:
            raise ValueError('by must be "max", "topk_mean" or "count" (got %r)' % (by,))
        score = score.cpu()
        score = torch.where(torch.isnan(score), torch.full_like(score, float("-inf")), score)
        order = torch.sort(score, descending=True, stable=True)[1].tolist()
        vals = score.tolist()
        return [(self.names[i], int(vals[i]) if by == "count" else vals[i]) for i in order]

    def find_objects(self, grid, thresholds, **kw):
        """The objects of this search's heat-map (openscene_amd.objects.find_objects over `grid`, a VoxelGrid of the bank's
        points): where in every scene the matches are, how many, how large.  Needs a search with return_heat."""
        if self.heat is None:
            raise ValueError("the search was run without return_heat")
        from .objects import find_objects
        kw.setdefault("names", self.names)
        return find_objects(grid, self.heat, thresholds, **kw)


def _queries(queries, dim, device):
    if not isinstance(queries, torch.Tensor):
        raise TypeError("queries must be a float16 tensor")
    if queries.dtype != torch.float16:
        raise TypeError("queries must be float16 (util/util.py:41-44 produces fp16); got %s" % queries.dtype)
    if queries.dim() != 2 or queries.shape[1] != dim:
        raise ValueError("queries must be [Q, %d] (got %s)" % (dim, tuple(queries.shape)))
    if queries.shape[0] < 1:
        raise ValueError("no query given")
    return queries.to(device)


def search(bank, queries, k=16, thresholds=None, normalize=True, return_heat=False):
    """Score every point of the bank against every query and select per scene.

    queries fp16 [Q, dim], L2-normalised (``util/util.py:41-44``); the score is ``run/evaluate.py:305,310`` (normalize:
    ``(hf / (hf.norm(dim=-1, keepdim=True) + 1e-5)).half() @ t.t()``) or ``:291`` (``h @ t.t()``) on the stored fp16
    rows.  thresholds: a number or [Q] numbers -> counts.  Selection order: higher score, then lower point index; NaN
    below every number."""
    if not isinstance(bank, FeatureBank):
        raise TypeError("bank must be a FeatureBank")
    queries = _queries(queries, bank.dim, bank.device)
    k = int(k)
    if not 1 <= k <= ops.BANK_MAX_K:
        raise ValueError("k must be in 1 .. %d (got %d)" % (ops.BANK_MAX_K, k))
    q = queries.shape[0]
    if thresholds is not None:
        thresholds = torch.as_tensor(thresholds, dtype=torch.float32).reshape(-1)
        if thresholds.numel() == 1 and q > 1:
            thresholds = thresholds.expand(q)
        if thresholds.numel() != q:
            raise ValueError("%d thresholds for %d queries" % (thresholds.numel(), q))
        thresholds = thresholds.contiguous().to(bank.device)
    rows = bank.scene_rows()
    heat, top_s, top_p, counts = ops.bank_search(bank.features, bank.offsets_tensor(), queries, k=k, thresholds=thresholds,
                                                 normalize=bool(normalize), want_heat=bool(return_heat),
                                                 max_scene_rows=max(rows) if rows else 0,
                                                 err=bank._err_word())       # (the bank owns its offsets: nothing to check)
    return SearchResult(bank.names, bank.offsets, top_s, top_p, counts, heat)


def heat_map(features, queries, inds_reverse=None, normalize=True):
    """fp16 [points, Q]: one scene's similarity heat-map (a bank of one scene)."""
    bank = FeatureBank(features.shape[1], features.device, capacity_rows=(inds_reverse if inds_reverse is not None else features).shape[0])
    bank.add_scene("scene", features, inds_reverse)
    return search(bank, queries, k=1, normalize=normalize, return_heat=True).heat
