"""The features themselves, before any prompt: second moments of a bank, principal feature directions and the picture
every user of an open-vocabulary feature field draws first -- the point cloud coloured by its first three principal
directions.  It shows whether fusion or distillation worked, where the model separates things and which scans are broken.

The rows are taken as the query scores them, ``(hf / (hf.norm(dim=-1, keepdim=True) + 1e-5)).half()``
(``run/evaluate.py:305,310``), or as they are stored (normalize=False):

    moments               bank (+ groups) -> Moments: count, sum, gram (= sum of h h^T) per group; .mean, .covariance()
    principal_directions  Moments -> Basis: the k leading eigenvectors per group (host, float64), variances, explained share
    Basis.project         coordinates of every bank row along the components (the search's heat pass: no new kernel)
    Basis.colors          uint8 [N, 3] between the lo / hi quantiles of each coordinate: what ``Raster.colors`` draws
    feature_colors        the three calls in one, for the whole bank or scene by scene

Kernels: csrc/gram.hip through ops.bank_gram / ops.bank_gram_fp8 (both bank kinds; an fp8 bank is never dequantised, no
[N, dim] temporary is made), csrc/search.hip for the projection; no CPU path.  The eigen-decomposition is one dim x dim
problem per group, done once per bank with torch.linalg.eigh on the host.
"""
import torch

from . import ops
from .descriptors import PointGroups
from .search import FeatureBank

MAX_GRAM_BYTES = 1 << 31         # moments() refuses a result beyond this


class Moments:
    """What `moments` returns: count int64 [G], sum float32 [G, dim], gram float32 [G, dim, dim] (bitwise symmetric), shape
    (the groups' logical shape), normalize (how the rows were taken), and
        mean     float32 [G, dim] = sum / count, zero for an empty group"""

    def __init__(self, count, total, gram, shape, normalize=True):
        self.count = count
        self.sum = total
        self.gram = gram
        self.shape = tuple(shape)
        self.normalize = bool(normalize)
        some = count > 0
        self.mean = torch.where(some[:, None], total / count.clamp(min=1).to(total.dtype)[:, None], torch.zeros_like(total))

    @property
    def dim(self):
        return self.sum.shape[1]

    def second_moment(self):
        """float64 [G, dim, dim] on the host: gram / count, zero for an empty group."""
        n = self.count.cpu().double().clamp(min=1)
        return self.gram.cpu().double() / n[:, None, None]

    def covariance(self):
        """float64 [G, dim, dim] on the host: gram / count - mean mean^T (the population covariance); a group of fewer
        than two rows gives zeros.  Synchronises."""
        count = self.count.cpu()
        mean = self.sum.cpu().double() / count.double().clamp(min=1)[:, None]
        cov = self.second_moment() - mean[:, :, None] * mean[:, None, :]
        cov[count < 2] = 0
        return cov


class Basis:
    """What `principal_directions` returns, per group: mean float32 [G, dim] (zeros when not centred), components float32
    [G, k, dim] (unit rows, descending variance, the entry of largest magnitude positive), variance float64 [G, k], total_variance
    float64 [G], explained = variance / total_variance, normalize (how the rows were taken).  All on the host."""

    def __init__(self, mean, components, variance, total_variance, normalize=True):
        self.mean = mean
        self.components = components
        self.variance = variance
        self.total_variance = total_variance
        self.normalize = bool(normalize)
        some = total_variance > 0
        self.explained = torch.where(some[:, None], variance / torch.where(some, total_variance, torch.ones_like(total_variance))[:, None],
                                     torch.zeros_like(variance))

    @property
    def k(self):
        return self.components.shape[1]

    def _rows(self, bank, scene):
        if not isinstance(bank, FeatureBank):
            raise TypeError("bank must be a FeatureBank")
        if bank.dim != self.components.shape[2]:
            raise ValueError("the basis has %d features, the bank %d" % (self.components.shape[2], bank.dim))
        if scene is None:
            return 0, bank.rows
        i = bank.names.index(scene) if isinstance(scene, str) else int(scene)
        if not 0 <= i < len(bank):
            raise IndexError("scene %d of %d" % (i, len(bank)))
        return bank.offsets[i], bank.offsets[i + 1]

    def project(self, bank, group=0, scene=None):
        """float32 [N, k] on the bank's device: the coordinates ``x . c_j - mean . c_j`` of every bank row (of one scene's rows
        with `scene`, a name or position) along the components of `group`, x the row as the basis was built (normalised or
        not).  The scores come from the search's heat pass with the components rounded to fp16 as queries -- fp16 scores --
        and the offset ``mean . c_j`` is taken on the same rounded components.  Synchronises once (the error word)."""
        group = int(group)
        if not 0 <= group < self.components.shape[0]:
            raise IndexError("group %d of %d" % (group, self.components.shape[0]))
        a, b = self._rows(bank, scene)
        dev = bank.device
        if b == a:
            return torch.zeros((0, self.k), dtype=torch.float32, device=dev)
        comps = self.components[group].half()
        offset = (comps.double() @ self.mean[group].double()).float()
        err = bank._err_word()
        kw = dict(k=1, normalize=self.normalize, want_heat=True, max_scene_rows=0, err=err)
        none = torch.zeros(1, dtype=torch.int64, device=dev)                # no scenes: the heat pass alone
        if bank.dtype == "fp8":
            heat = ops.bank_search_fp8(bank.codes[a:b], bank.exponents[a:b], none, comps.to(dev), **kw)[0]
        else:
            heat = ops.bank_search(bank.features[a:b], none, comps.to(dev), **kw)[0]
        bank._checked(err)
        return heat.float() - offset.to(dev)

    def colors(self, bank, group=0, lo=0.01, hi=0.99, scene=None):
        """uint8 [N, 3] on the bank's device, ready for ``Raster.colors``: each of the first three coordinates of `project`
        mapped affinely from its [lo, hi] quantiles (the sorted values at rint(q (N - 1))) to 0 .. 255, clamped and rounded
        to nearest; a constant coordinate (and a NaN) gives 128."""
        if self.k < 3:
            raise ValueError("colours need three components (the basis has %d)" % self.k)
        lo, hi = float(lo), float(hi)
        if not 0.0 <= lo < hi <= 1.0:
            raise ValueError("need 0 <= lo < hi <= 1 (got %r, %r)" % (lo, hi))
        xy = self.project(bank, group, scene)[:, :3]
        n = xy.shape[0]
        if n == 0:
            return torch.zeros((0, 3), dtype=torch.uint8, device=xy.device)
        ranked = torch.sort(xy, dim=0)[0]
        a = ranked[int(round(lo * (n - 1)))]
        b = ranked[int(round(hi * (n - 1)))]
        flat = ~(b > a)
        span = torch.where(flat, torch.ones_like(b), b - a)
        v = torch.round(((xy - a) / span).clamp(0, 1) * 255)
        v = torch.where(flat[None, :] | torch.isnan(v), torch.full_like(v, 128), v)
        return v.to(torch.uint8)


def moments(bank, groups=None, normalize=True):
    """Count, sum and Gram matrix of the rows of `bank` (either kind) per point set of `groups` (a PointGroups; None: the
    whole bank is one group; ``PointGroups.from_scenes(bank)``: one per scene), the rows taken as
    ``(hf / (hf.norm(dim=-1, keepdim=True) + 1e-5)).half()`` (``run/evaluate.py:305,310``; normalize=False: as stored, rounded
    to fp16).  A row outside the bank raises (``ops.bank_check``) and leaves the bank usable.  Synchronises once."""
    if not isinstance(bank, FeatureBank):
        raise TypeError("bank must be a FeatureBank")
    if groups is None:
        groups = PointGroups(torch.tensor([0, bank.rows], dtype=torch.int64).to(bank.device), None, (1,), n_entries=bank.rows,
                             _checked=True)
    if not isinstance(groups, PointGroups):
        raise TypeError("groups must be a PointGroups or None")
    if bank.dim > ops.BANK_POOL_MAX_DIM:
        raise ValueError("rows of up to %d features can be taken moments of (the bank has %d)" % (ops.BANK_POOL_MAX_DIM, bank.dim))
    if groups.device != bank.device:
        raise ValueError("the groups must be on the bank's device (%s, got %s)" % (bank.device, groups.device))
    size = groups.n_groups * bank.dim * bank.dim * 4
    if size > MAX_GRAM_BYTES:
        raise ValueError("%d groups x %d x %d float32 are %d bytes (%.2f GiB): more than the %d GiB a call returns; take the groups in parts"
                         % (groups.n_groups, bank.dim, bank.dim, size, size / 2.0 ** 30, MAX_GRAM_BYTES >> 30))
    err = bank._err_word()
    kw = dict(rows=groups.rows, normalize=bool(normalize), n_entries=groups.n_entries, err=err)
    if bank.dtype == "fp8":
        gram, total, count = ops.bank_gram_fp8(bank.codes, bank.exponents, groups.starts, **kw)
    else:
        gram, total, count = ops.bank_gram(bank.features, groups.starts, **kw)
    bank._checked(err)
    return Moments(count, total, gram, groups.shape, normalize)


def principal_directions(moments, k=3, center=True):
    """The k leading principal directions of every group of a Moments: eigenvectors of the covariance (center=True) or of the
    second moment gram / count (center=False: the first direction is then close to the mean direction), by
    ``torch.linalg.eigh`` in float64.  SYNCHRONISES AND RUNS ON THE CPU: one dim x dim problem per group, done once per
    bank.  Components in descending eigenvalue order; sign: the entry of largest magnitude is positive, the lowest index
    wins ties -- this fixes the colours.  -> Basis"""
    if not isinstance(moments, Moments):
        raise TypeError("moments must be a Moments")
    k = int(k)
    d = moments.dim
    if not 1 <= k <= d:
        raise ValueError("k must be in 1 .. %d (got %d)" % (d, k))
    m = moments.covariance() if center else moments.second_moment()
    m = torch.nan_to_num(m, nan=0.0, posinf=0.0, neginf=0.0)                     # (a NaN group has no directions: zeros, variance 0)
    g = m.shape[0]
    if g:
        vals, vecs = torch.linalg.eigh(m)                                       # ascending
        vals = vals.flip(-1)[:, :k].clamp(min=0)
        comps = vecs.flip(-1)[:, :, :k].transpose(1, 2).contiguous()            # [G, k, d]
    else:
        vals, comps = torch.zeros(0, k, dtype=torch.float64), torch.zeros(0, k, d, dtype=torch.float64)
    top = comps.abs().argmax(dim=-1, keepdim=True)                              # (argmax returns the first of equal maxima)
    sign = torch.where(torch.gather(comps, -1, top) < 0, -1.0, 1.0).to(comps.dtype)
    comps = comps * sign
    total = torch.diagonal(m, dim1=-2, dim2=-1).sum(-1).clamp(min=0)
    mean = moments.mean.cpu().float() if center else torch.zeros(g, d, dtype=torch.float32)
    return Basis(mean, comps.float(), vals, total, moments.normalize)


def feature_colors(bank, per_scene=False, normalize=True, lo=0.01, hi=0.99):
    """uint8 [N, 3]: every bank row coloured by its coordinates along the first three principal feature directions --
    `moments`, `principal_directions`, `Basis.colors` in one.  per_scene: every scene gets its own basis and its own
    quantiles (its rows are written scene by scene), else one basis for the whole bank."""
    if not isinstance(bank, FeatureBank):
        raise TypeError("bank must be a FeatureBank")
    if not per_scene:
        return principal_directions(moments(bank, None, normalize), 3).colors(bank, 0, lo, hi)
    basis = principal_directions(moments(bank, PointGroups.from_scenes(bank), normalize), 3)
    out = torch.empty((bank.rows, 3), dtype=torch.uint8, device=bank.device)
    for s in range(len(bank)):
        out[bank.offsets[s]:bank.offsets[s + 1]] = basis.colors(bank, s, lo, hi, scene=s)
    return out
