"""Search a bank of scenes by text (or image) embedding: the reference README's "Applications" -- scene exploration by
free text, rare object search in a 3D scene database, image-based retrieval -- on per-point OpenScene features.

The reference forms the features (``run/evaluate.py:290`` distill, ``:285`` fusion, ``:318`` ensemble), scores them
against CLIP text embeddings (``:291``, ``:305,310``) and can save them per scene (``save_feature_as_numpy``,
``:232-235,328-330``: ``<scene>_openscene_feat_<feature_type>.npy``).  Here:

    FeatureBank      one growing matrix of per-point features, many scenes, on the device: fp16, or fp8 (e4m3fn codes
                     with one power-of-two exponent per row) at half the bytes
    search           heat-map [N, Q] + the k best points of every scene + counts over a threshold: ONE pass over the bank;
                     with negative queries the scores are relevancies against the best negative (same pass)
    heat_map         the one-scene convenience
    SearchResult     .rank_scenes(q, by=...) orders the scenes for a query; .find_objects(grid, thresholds) groups the
                     heat-map into ranked objects (openscene_amd.objects); .render(raster, scene, q) draws a heat column
                     over rendered views of the scene (openscene_amd.render)

Kernels: csrc/search.hip through ops.bank_append / ops.bank_search and their _fp8 twins (osn_bank_search_contrast[_fp8]
when negatives are given, osn_bank_search_ensemble[_fp8] when a second bank is); no CPU path.
"""
import numpy as np
import torch

from . import io as _io
from . import ops


# what a bank of each kind stores: (name in the file, dtype, a row is [dim] values (True) or one (False)) per tensor
_STORAGE = {"fp16": (("features", torch.float16, True),),
            "fp8": (("codes", torch.uint8, True), ("exponents", torch.int8, False))}


class FeatureBank:
    """A growing [rows, dim] matrix on `device` holding the per-point features of many scenes back to back.

    dtype    "fp16": the rows as ``run/evaluate.py:291`` scores them (``.half()``), two bytes per element.
             "fp8": one byte per element -- OCP e4m3fn codes (uint8 [rows, dim]) and one power-of-two exponent per row
             (int8 [rows]); a stored value is ``code * 2^e`` (include/openscene_amd.h states the format bit for bit).
             Twice the scenes in the same memory, half the bytes for the search to stream.
    offsets  python list, S + 1 ascending row offsets (scene i is rows offsets[i] : offsets[i + 1])
    names    python list of the S scene names (unique)
    """

    def __init__(self, dim, device, capacity_rows=1 << 16, dtype="fp16"):
        dim = int(dim)
        if dtype not in ("fp16", "fp8"):
            raise ValueError('dtype must be "fp16" or "fp8" (got %r)' % (dtype,))
        if dtype == "fp8" and (dim < 16 or dim % 16):
            raise ValueError("dim of an fp8 bank must be a positive multiple of 16 (got %d)" % dim)
        if dim < 8 or dim % 8:
            raise ValueError("dim must be a positive multiple of 8 (got %d)" % dim)
        self.dim = dim
        self.dtype = dtype
        self.device = torch.device(device)
        self._store = self._alloc(max(int(capacity_rows), 1))          # (features,) or (codes, exponents), filled and scratch rows
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
        return self._store[0].shape[0]

    @property
    def nbytes(self):
        """Bytes of the filled rows."""
        return self.rows * sum(t.element_size() * t[0].numel() for t in self._store)

    def _need(self, dtype, what):
        if self.dtype != dtype:
            hint = "; dequantize(which=None) returns its values as float32" if self.dtype == "fp8" else ""
            raise TypeError("%s is for an %s bank, this one is %s%s" % (what, dtype, self.dtype, hint))

    @property
    def features(self):
        """fp16 [rows, dim]: a view of the filled part (fp16 bank)."""
        self._need("fp16", "features")
        return self._store[0][:self.rows]

    @property
    def codes(self):
        """uint8 [rows, dim]: the e4m3fn codes of the filled part (fp8 bank)."""
        self._need("fp8", "codes")
        return self._codes[:self.rows]

    @property
    def exponents(self):
        """int8 [rows]: the row exponents of the filled part (fp8 bank)."""
        self._need("fp8", "exponents")
        return self._exps[:self.rows]

    @property
    def _codes(self):
        return self._store[0]

    @property
    def _exps(self):
        return self._store[1]

    def _span(self, which):
        if which is None:
            return 0, self.rows
        i = self.names.index(which) if isinstance(which, str) else int(which)
        return self.offsets[i], self.offsets[i + 1]

    def scene(self, which):
        """fp16 [n, dim] view of one scene's rows (by name or position; fp16 bank)."""
        self._need("fp16", "scene()")
        a, b = self._span(which)
        return self._store[0][a:b]

    def dequantize(self, which=None):
        """float32 [n, dim]: the stored values ``code * 2^e`` of one scene (by name or position) or, with None, of the
        whole fp8 bank.  Plain torch: for inspection and tests, not for the search."""
        self._need("fp8", "dequantize()")
        a, b = self._span(which)
        table = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().to(self.device)
        return torch.ldexp(table[self._codes[a:b].long()], self._exps[a:b].int()[:, None])

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
    def _alloc(self, cap):
        return tuple(torch.empty((cap, self.dim) if wide else (cap,), dtype=dtype, device=self.device)
                     for _, dtype, wide in _STORAGE[self.dtype])

    def _reserve(self, n):
        need = self.rows + n
        if need <= self.capacity_rows:
            return
        store = self._alloc(max(need, 2 * self.capacity_rows))
        for new, old in zip(store, self._store):
            new[:self.rows].copy_(old[:self.rows])
        self._store = store

    def _commit(self, name, n):
        self.offsets.append(self.rows + n)
        self.names.append(name)
        self._offsets_dev = None

    def _gather(self, inds_reverse):
        inds_reverse = torch.as_tensor(inds_reverse).to(self.device)
        if inds_reverse.dim() != 1 or inds_reverse.dtype.is_floating_point or inds_reverse.dtype == torch.bool:
            raise TypeError("inds_reverse must be a vector of integer indices")
        return inds_reverse

    def _checked(self, err):
        try:
            ops.bank_check(err)
        except Exception:
            err.zero_()                           # rows past `rows` are scratch: the bank is as it was
            raise

    def _append(self, features, inds_reverse):
        """features[inds_reverse] through the bank kind's append kernel into the rows after the filled ones.  -> their number"""
        features = features.to(self.device)
        if inds_reverse is not None:
            inds_reverse = self._gather(inds_reverse)
        n = features.shape[0] if inds_reverse is None else inds_reverse.shape[0]
        self._reserve(n)
        err = self._err_word()
        append = ops.bank_append if self.dtype == "fp16" else ops.bank_append_fp8
        append(*self._store, self.rows, features, err, gather=inds_reverse)
        self._checked(err)
        return n

    def add_scene(self, name, features, inds_reverse=None):
        """Append one scene.  float32 features on the bank's device -- the network output, with the voxel -> point
        map `inds_reverse`: exactly ``predictions = feat_3d[inds_reverse]`` of ``run/evaluate.py:290``, stored as the
        ``.half()`` of ``:291`` -- go through the fused gather + cast kernel; fp16 features (fused / ensemble features,
        saved files) are copied as they are.  An fp8 bank sends both kinds through the gather + quantise kernel.  An
        index outside the feature matrix raises and leaves the bank as it was.  -> the scene's position."""
        name = str(name)
        if name in self.names:
            raise ValueError("the bank already holds a scene named %r" % name)
        if isinstance(features, np.ndarray):
            features = torch.from_numpy(features)
        if features.dim() != 2 or features.shape[1] != self.dim:
            raise ValueError("features must be [points, %d] (got %s)" % (self.dim, tuple(features.shape)))
        if features.dtype not in (torch.float16, torch.float32):
            raise TypeError("features must be float32 or float16 (got %s)" % features.dtype)
        if self.dtype == "fp16" and features.dtype == torch.float16:
            rows = features if inds_reverse is None else features[torch.as_tensor(inds_reverse).long().to(features.device)]
            n = rows.shape[0]
            self._reserve(n)
            self._store[0][self.rows:self.rows + n].copy_(rows)
        else:
            n = self._append(features, inds_reverse)
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

    def to_fp8(self):
        """The fp8 bank of the same scenes: this fp16 bank's rows through the quantising kernel."""
        self._need("fp16", "to_fp8()")
        bank = FeatureBank(self.dim, self.device, capacity_rows=max(self.rows, 1), dtype="fp8")
        if self.rows:
            bank._append(self.features, None)
        bank.offsets = list(self.offsets)
        bank.names = list(self.names)
        return bank

    def select(self, other, source):
        """A new bank of the same kind and scenes whose row p is `other`'s where ``source[p]`` is true and this bank's
        elsewhere: the reference's ``feat_ensemble`` (``run/evaluate.py:318-324``, "if we need to save the features") for the
        label set `source` was chosen with -- ``search(..., ensemble=other).source`` in vocabulary mode.  fp16 rows are
        copied; fp8 rows copy codes and exponent byte.  Ready for save, io.save_point_features, pool and pca."""
        _same_banks(self, other)
        if not isinstance(source, torch.Tensor) or source.dtype != torch.bool or tuple(source.shape) != (self.rows,):
            raise ValueError("source must be a bool [%d] tensor (the .source of a vocabulary-mode search)" % self.rows)
        source = source.to(self.device)
        bank = FeatureBank(self.dim, self.device, capacity_rows=max(self.rows, 1), dtype=self.dtype)
        for dst, mine, theirs in zip(bank._store, self._store, other._store):
            pick = source[:, None] if mine.dim() == 2 else source
            dst[:self.rows].copy_(torch.where(pick, theirs[:self.rows], mine[:self.rows]))
        bank.offsets = list(self.offsets)
        bank.names = list(self.names)
        return bank

    # ---- persistence
    def save(self, path):
        """One file: the filled rows (fp16, or codes and exponents), the offsets and the names."""
        d = {"dim": self.dim, "offsets": list(self.offsets), "names": list(self.names), "dtype": self.dtype}
        for (key, _, _), t in zip(_STORAGE[self.dtype], self._store):
            d[key] = t[:self.rows].cpu().clone()
        torch.save(d, path)

    @classmethod
    def load(cls, path, device):
        d = torch.load(path, map_location="cpu", weights_only=False)
        dtype = d.get("dtype", "fp16")                      # (files written before the fp8 bank hold no "dtype")
        rows = d["offsets"][-1]
        layout = _STORAGE.get(dtype, ())
        parts = [d.get(key) for key, _, _ in layout]
        if not parts or any(t is None or t.dtype != dt or tuple(t.shape) != ((rows, d["dim"]) if wide else (rows,))
                            for t, (_, dt, wide) in zip(parts, layout)):
            raise ValueError("%s is not a feature bank" % path)
        bank = cls(d["dim"], device, capacity_rows=max(rows, 1), dtype=dtype)
        for dst, t in zip(bank._store, parts):
            dst[:rows].copy_(t)
        bank.offsets = [int(o) for o in d["offsets"]]
        bank.names = [str(n) for n in d["names"]]
        return bank


def _same_banks(a, b):
    """Two banks that can be searched as one: raises ValueError naming the first difference."""
    if not isinstance(b, FeatureBank):
        raise TypeError("ensemble must be a FeatureBank")
    if b.dtype != a.dtype:
        raise ValueError("the two banks differ in kind: %s and %s (mixed kinds are not supported)" % (a.dtype, b.dtype))
    if b.dim != a.dim:
        raise ValueError("the two banks differ in dim: %d and %d" % (a.dim, b.dim))
    if b.device != a.device:
        raise ValueError("the two banks differ in device: %s and %s" % (a.device, b.device))
    if b.names != a.names:
        raise ValueError("the two banks differ in scene names: %r and %r"
                         % next(((x, y) for x, y in zip(a.names, b.names) if x != y), (len(a.names), len(b.names))))
    if b.offsets != a.offsets:
        raise ValueError("the two banks differ in scene offsets: %r and %r" % (a.offsets, b.offsets))


class SearchResult:
    """topk_scores fp16 [S, Q, k], topk_points int64 [S, Q, k] (row inside its scene; -1 with score -inf pads a scene
    of fewer than k points), counts int64 [S, Q] or None (points with score >= the query's threshold), heat fp16 [N, Q]
    or None, names (the bank's scene names), offsets.  relevancy: the search was given negatives -- every score (heat,
    topk_scores, what thresholds and counts compare) is then the relevancy in [0, 1] against the best negative at
    `temperature` (None for a plain search), and 0.5 means "as likely as the best negative".  source / ensemble_mode: the
    search was given a second bank (``ensemble=``) -- source is bool [N] in "vocabulary" mode (the point's row comes from the
    second bank), bool [N, Q] in "query" mode with return_heat (the element does); both None for every other search."""

    def __init__(self, names, offsets, topk_scores, topk_points, counts, heat, relevancy=False, temperature=None, source=None,
                 ensemble_mode=None):
        self.names = list(names)
        self.offsets = list(offsets)
        self.topk_scores = topk_scores
        self.topk_points = topk_points
        self.counts = counts
        self.heat = heat
        self.relevancy = bool(relevancy)
        self.temperature = temperature
        self.source = source
        self.ensemble_mode = ensemble_mode

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
        points): where in every scene the matches are, how many, how large.  Needs a search with return_heat.  After a
        search with negatives the thresholds are relevancies: 0.5 means "as likely as the best negative", for every query."""
        if self.heat is None:
            raise ValueError("the search was run without return_heat")
        from .objects import find_objects
        kw.setdefault("names", self.names)
        return find_objects(grid, self.heat, thresholds, **kw)

    def near(self, grid, target, anchor, anchor_threshold, distance, reach=None):
        """"target near anchor": fp16 [N, 1], column `target` of this search's heat-map where the point's voxel lies within
        `distance` of a voxel holding a hit of column `anchor` (score >= anchor_threshold), -inf elsewhere
        (openscene_amd.reach.near over `grid`, a VoxelGrid of the bank's points).  Needs a search with return_heat."""
        if self.heat is None:
            raise ValueError("the search was run without return_heat")
        from .reach import near
        return near(grid, self.heat, target, anchor, anchor_threshold, distance, reach=reach)

    def render(self, raster, scene, q, lo=None, hi=None, base=None, **kw):
        """uint8 [V, H, W, 3]: the views of `raster` (openscene_amd.render.rasterize of that scene's points) shaded with
        column q of the scene's heat-map, read in place through the row stride.  After a search with negatives the
        defaults are lo = 0.5 ("as likely as the best negative") and hi = 1; plain scores have no natural range: lo and hi
        are required.  base uint8 [n, 3]: the points below lo keep their own colour and the hits stand out, the demo's
        look.  Needs a search with return_heat."""
        heat = self.scene_heat(scene)
        q = int(q)
        if not 0 <= q < heat.shape[1]:
            raise IndexError("query %d of %d" % (q, heat.shape[1]))
        if heat.shape[0] != raster.n:
            raise ValueError("the scene has %d points but the raster was drawn from %d" % (heat.shape[0], raster.n))
        if self.relevancy:
            lo, hi = (0.5 if lo is None else lo), (1.0 if hi is None else hi)
        elif lo is None or hi is None:
            raise ValueError("lo and hi are required for plain scores (only relevancies have the default range 0.5 .. 1)")
        return raster.heat(heat, lo, hi, base=base, column=q, **kw)


def _queries(queries, dim, device, what="queries", letter="Q"):
    if not isinstance(queries, torch.Tensor):
        raise TypeError("%s must be a float16 tensor" % what)
    if queries.dtype != torch.float16:
        raise TypeError("%s must be float16 (util/util.py:41-44 produces fp16); got %s" % (what, queries.dtype))
    if queries.dim() != 2 or queries.shape[1] != dim:
        raise ValueError("%s must be [%s, %d] (got %s)" % (what, letter, dim, tuple(queries.shape)))
    if queries.shape[0] < 1:
        raise ValueError("no %s given" % what)
    return queries.to(device)


def search(bank, queries, k=16, thresholds=None, normalize=True, return_heat=False, negatives=None, temperature=0.1,
           ensemble=None, ensemble_mode="vocabulary"):
    """Score every point of the bank against every query and select per scene.

    queries fp16 [Q, dim], L2-normalised (``util/util.py:41-44``); the score is ``run/evaluate.py:305,310`` (normalize:
    ``(hf / (hf.norm(dim=-1, keepdim=True) + 1e-5)).half() @ t.t()``) or ``:291`` (``h @ t.t()``) on the stored fp16
    rows (an fp8 bank: on its stored values ``code * 2^e``).  thresholds: a number or [Q] numbers -> counts.  Selection
    order: higher score, then lower point index; NaN below every number.

    negatives fp16 [M, dim], L2-normalised like the queries ("object", "things", "stuff", "texture" are the usual ones):
    every score becomes the relevancy ``sigmoid((score - best negative score of the point) / temperature)`` -- the
    smallest pairwise softmax of the query against a negative -- in the same pass over the bank; the heat-map, the
    top-k, thresholds and counts are all taken on it, and a threshold of 0.5 means "as likely as the best negative"
    for every query.  The negatives get no column of their own.  temperature: finite and > 0; the default 0.1 is an
    interface default, not a tuned value.

    ensemble: a second FeatureBank of the same kind, dim, device and scenes (equal names and offsets) -- in the reference
    `bank` holds the distilled features and `ensemble` the fused ones -- searched with `bank` as one, the 2D-3D ensemble of
    ``run/evaluate.py:302-324`` at query time, in the pass that reads the two banks:
      ensemble_mode="vocabulary" (``:318-321``)  a point takes its whole row from the source whose best normalised score over
        THIS CALL'S queries is larger (the second bank only if strictly larger; always on normalised scores, whatever
        `normalize`; negatives take no part).  A query's column therefore depends on the other queries of the call.
      ensemble_mode="query" (the commented variant, ``:312-316``)  every element is the larger of the two sources' scores
        (relevancies with negatives); column q depends on query q alone.
    The result's .source says which (bool [N], or bool [N, Q] with return_heat); top-k, thresholds and counts are taken on the
    combined heat-map.  bank.select(ensemble, source) stores the vocabulary-mode choice as a bank of its own."""
    if not isinstance(bank, FeatureBank):
        raise TypeError("bank must be a FeatureBank")
    if ensemble is not None:
        _same_banks(bank, ensemble)
        if ensemble_mode not in ops.BANK_ENSEMBLE_MODES:
            raise ValueError('ensemble_mode must be "vocabulary" or "query" (got %r)' % (ensemble_mode,))
    queries = _queries(queries, bank.dim, bank.device)
    contrast = {}
    if negatives is not None:
        temperature = float(temperature)
        if not 0.0 < temperature < float("inf"):                 # (NaN fails both comparisons)
            raise ValueError("temperature must be finite and > 0 (got %r)" % (temperature,))
        contrast = dict(negatives=_queries(negatives, bank.dim, bank.device, "negatives", "M"), temperature=temperature)
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
    kw = dict(k=k, thresholds=thresholds, normalize=bool(normalize), want_heat=bool(return_heat),
              max_scene_rows=max(rows) if rows else 0, err=bank._err_word())       # (the bank owns its offsets: nothing to check)
    source = None
    if ensemble is not None:
        kw.update(mode=ensemble_mode, want_source=bool(return_heat))
        if bank.dtype == "fp8":
            heat, top_s, top_p, counts, source = ops.bank_search_ensemble_fp8(
                bank.codes, bank.exponents, ensemble.codes, ensemble.exponents, bank.offsets_tensor(), queries, **kw, **contrast)
        else:
            heat, top_s, top_p, counts, source = ops.bank_search_ensemble(bank.features, ensemble.features, bank.offsets_tensor(),
                                                                          queries, **kw, **contrast)
    elif bank.dtype == "fp8":
        heat, top_s, top_p, counts = ops.bank_search_fp8(bank.codes, bank.exponents, bank.offsets_tensor(), queries, **kw, **contrast)
    else:
        heat, top_s, top_p, counts = ops.bank_search(bank.features, bank.offsets_tensor(), queries, **kw, **contrast)
    return SearchResult(bank.names, bank.offsets, top_s, top_p, counts, heat, relevancy=bool(contrast),
                        temperature=contrast.get("temperature"), source=source,
                        ensemble_mode=ensemble_mode if ensemble is not None else None)


def heat_map(features, queries, inds_reverse=None, normalize=True, negatives=None, temperature=0.1, ensemble=None,
             ensemble_mode="vocabulary"):
    """fp16 [points, Q]: one scene's similarity heat-map (a bank of one scene); with negatives, its relevancy map (search).
    ensemble: a second feature matrix per voxel, like `features` (same rows, width and device; it goes through the same
    `inds_reverse`, ``run/evaluate.py:303,308``): the heat-map of the two as one (search's `ensemble`)."""
    rows = (inds_reverse if inds_reverse is not None else features).shape[0]
    bank = FeatureBank(features.shape[1], features.device, capacity_rows=rows)
    bank.add_scene("scene", features, inds_reverse)
    other = None
    if ensemble is not None:
        if isinstance(ensemble, np.ndarray):
            ensemble = torch.from_numpy(ensemble)
        if not isinstance(ensemble, torch.Tensor) or ensemble.dim() != 2:
            raise TypeError("ensemble must be a [rows, dim] feature matrix")
        if tuple(ensemble.shape) != tuple(features.shape) or ensemble.device != features.device:
            raise ValueError("ensemble must be %s on %s, like features (got %s on %s)"
                             % (tuple(features.shape), features.device, tuple(ensemble.shape), ensemble.device))
        other = FeatureBank(features.shape[1], features.device, capacity_rows=rows)
        other.add_scene("scene", ensemble, inds_reverse)
    return search(bank, queries, k=1, normalize=normalize, return_heat=True, negatives=negatives, temperature=temperature,
                  ensemble=other, ensemble_mode=ensemble_mode).heat
