"""From points back to a feature vector: descriptors of scenes, objects and regions of a bank -- the other half of the
reference README's "Applications": "retrieve examples based on similarities" (an object found by `find_objects` becomes the
next query), room type (one descriptor per scene scored against a prompt set), and labelling a found object or a selected
region against a vocabulary.

A descriptor is the mean of the normalised feature rows of a point set, the normalisation that of ``run/evaluate.py:305``
(``hf / (hf.norm(dim=-1, keepdim=True) + 1e-5)``):

    PointGroups      point sets in CSR form: .from_scenes(bank), .from_labels(labels, G), .from_lists([...]),
                     .from_objects(object_result)
    pool             bank + groups (+ weights) -> Descriptors
    Descriptors      .mean [G, dim], .count, .weight, .view(), .queries() (fp16, L2-normalised: ready for `search`)
    describe_scenes  one descriptor per scene of the bank

Kernels: csrc/pool.hip through ops.bank_pool / ops.bank_pool_fp8 (both bank kinds; an fp8 bank is never dequantised);
no CPU path.  The CSR arrays are built with torch.
"""
import torch

from . import ops
from .search import FeatureBank


def _prod(shape):
    p = 1
    for s in shape:
        p *= s
    return p


class PointGroups:
    """G point sets over the rows of a bank.

    starts     int64 [G + 1], ascending from 0 to L: group g holds the entries starts[g] : starts[g + 1]
    rows       int64 [L] bank rows, or None: entry i is bank row i (whole scenes need no index array)
    shape      the logical shape of the groups, product G (``Descriptors.view`` reshapes to it)
    n_entries  L
    query      int64 [L] or None: the heat-map column an entry was a hit of (`from_objects`)
    Order inside a group is accumulation order; a row may appear more than once."""

    def __init__(self, starts, rows=None, shape=None, n_entries=None, query=None, _checked=False):
        if not isinstance(starts, torch.Tensor) or starts.dtype != torch.int64 or starts.dim() != 1 or starts.shape[0] < 1:
            raise TypeError("starts must be an int64 [G + 1] tensor")
        if rows is not None and (not isinstance(rows, torch.Tensor) or rows.dtype != torch.int64 or rows.dim() != 1):
            raise TypeError("rows must be an int64 [L] tensor or None")
        if rows is not None and rows.device != starts.device:
            raise ValueError("starts and rows must be on one device")
        g = starts.shape[0] - 1
        shape = (g,) if shape is None else tuple(int(s) for s in shape)
        if any(s < 0 for s in shape) or _prod(shape) != g:
            raise ValueError("shape %s does not hold %d groups" % (shape, g))
        if not _checked:                                      # (the constructors below build their arrays: nothing to read back)
            host = starts.tolist()
            if host[0] != 0 or any(b < a for a, b in zip(host[:-1], host[1:])):
                raise ValueError("starts must ascend from 0")
            if rows is not None and host[-1] != rows.shape[0]:
                raise ValueError("starts must end at the number of rows (%d, got %d)" % (rows.shape[0], host[-1]))
            if n_entries is not None and host[-1] != int(n_entries):
                raise ValueError("starts must end at n_entries (%d, got %d)" % (int(n_entries), host[-1]))
            n_entries = host[-1]
        self.starts = starts.contiguous()
        self.rows = rows.contiguous() if rows is not None else None
        self.shape = shape
        self.n_entries = int(rows.shape[0] if rows is not None else n_entries)
        self.query = query

    @property
    def n_groups(self):
        return self.starts.shape[0] - 1

    @property
    def device(self):
        return self.starts.device

    @classmethod
    def from_scenes(cls, bank):
        """One group per scene of the bank, in scene order; no index array."""
        if not isinstance(bank, FeatureBank):
            raise TypeError("bank must be a FeatureBank")
        return cls(bank.offsets_tensor(), None, (len(bank),), n_entries=bank.rows, _checked=True)

    @classmethod
    def from_labels(cls, labels, n_groups):
        """labels: integers [N], one per bank row; label g puts the row into group g, -1 into none.  Rows ascend inside a group."""
        if not isinstance(labels, torch.Tensor) or labels.dim() != 1 or labels.dtype.is_floating_point or labels.dtype == torch.bool:
            raise TypeError("labels must be a vector of integers")
        n_groups = int(n_groups)
        if n_groups < 0:
            raise ValueError("n_groups must not be negative (got %d)" % n_groups)
        labels = labels.long()
        if labels.numel() and (int(labels.min()) < -1 or int(labels.max()) >= n_groups):
            raise ValueError("labels must lie in -1 .. %d" % (n_groups - 1))
        rows = torch.nonzero(labels >= 0).reshape(-1)
        lab = labels[rows]
        order = torch.sort(lab, stable=True)[1]
        return cls(_starts(lab, n_groups), rows[order], (n_groups,), _checked=True)

    @classmethod
    def from_lists(cls, lists, device=None):
        """One group per index tensor (or list of ints) of `lists`: arbitrary point sets, order and duplicates kept."""
        lists = [torch.as_tensor(x) for x in lists]
        lists = [x.long() if x.numel() == 0 else x for x in lists]             # (an empty python list has no integer dtype)
        for x in lists:
            if x.dim() != 1 or x.dtype.is_floating_point or x.dtype == torch.bool:
                raise TypeError("every point set must be a vector of integer indices")
        if device is None:
            device = lists[0].device if lists else torch.device("cpu")
        starts = [0]
        for x in lists:
            starts.append(starts[-1] + x.shape[0])
        rows = torch.cat([x.long().to(device) for x in lists]) if lists else torch.empty(0, dtype=torch.int64, device=device)
        return cls(torch.tensor(starts, dtype=torch.int64).to(device), rows, (len(lists),), _checked=True)

    @classmethod
    def from_objects(cls, result):
        """The kept objects of a ``find_objects(..., return_point_ids=True)`` result: shape (S, Q, M), group
        ((scene * Q) + q) * M + rank holds the hits of that object as bank rows (scene offset + point), ascending."""
        po = getattr(result, "point_object", None)
        if po is None:
            raise ValueError("the objects were found without return_point_ids: there is no point -> object map to pool over")
        s_n, q_n, m = result.n_points.shape
        dev = po.device
        hit = torch.nonzero(po >= 0)                            # (row, query) pairs, rows ascending
        rows, q = hit[:, 0], hit[:, 1]
        offs = torch.tensor(result.offsets, dtype=torch.int64).to(dev)
        scene = torch.bucketize(rows, offs[1:], right=True)     # the scene whose row range holds the row
        gid = (scene * q_n + q) * m + po[rows, q].long()
        order = torch.sort(gid, stable=True)[1]
        return cls(_starts(gid, s_n * q_n * m), rows[order], (s_n, q_n, m), query=q[order], _checked=True)


def _starts(group_of_entry, n_groups):
    counts = torch.bincount(group_of_entry, minlength=n_groups)
    starts = torch.zeros(n_groups + 1, dtype=torch.int64, device=group_of_entry.device)
    starts[1:] = torch.cumsum(counts, 0)
    return starts


class Descriptors:
    """What `pool` returns: sum float32 [G, dim] (the kernel's), weight float32 [G] (the groups' summed weights; the number
    of entries without weights), count int64 [G] (entries), shape (the groups' logical shape), and
        mean     float32 [G, dim] = sum / weight, zero where the weight is zero"""

    def __init__(self, total, weight, count, shape):
        self.sum = total
        self.weight = weight
        self.count = count
        self.shape = tuple(shape)
        some = weight > 0
        self.mean = torch.where(some[:, None], total / torch.where(some, weight, torch.ones_like(weight))[:, None],
                                torch.zeros_like(total))

    @property
    def dim(self):
        return self.sum.shape[1]

    def view(self):
        """mean with the leading axis reshaped to `shape`: [*shape, dim]."""
        return self.mean.reshape(self.shape + (self.dim,))

    def queries(self):
        """fp16 [G, dim]: the means L2-normalised as ``util/util.py:41-44`` normalises text embeddings
        (``f / f.norm(dim=-1, keepdim=True)``), zero rows left zero -- what `search` takes as queries."""
        norm = self.mean.norm(dim=-1, keepdim=True)
        return torch.where(norm > 0, self.mean / torch.where(norm > 0, norm, torch.ones_like(norm)),
                           torch.zeros_like(self.mean)).half()


def pool(bank, groups, weights=None, normalize=True):
    """Descriptors of the point sets `groups` over `bank` (either kind): per group the weighted mean of
    ``hf / (hf.norm(dim=-1, keepdim=True) + 1e-5)`` (``run/evaluate.py:305``; normalize=False: of the stored rows themselves).
    weights: float32 [L], one per entry, >= 0 and finite, or None.  A row outside the bank or a bad weight raises
    (``ops.bank_check``) and leaves the bank usable.  Synchronises once."""
    if not isinstance(bank, FeatureBank):
        raise TypeError("bank must be a FeatureBank")
    if not isinstance(groups, PointGroups):
        raise TypeError("groups must be a PointGroups")
    if bank.dim > ops.BANK_POOL_MAX_DIM:
        raise ValueError("rows of up to %d features can be pooled (the bank has %d)" % (ops.BANK_POOL_MAX_DIM, bank.dim))
    if groups.device != bank.device:
        raise ValueError("the groups must be on the bank's device (%s, got %s)" % (bank.device, groups.device))
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32:
            raise TypeError("weights must be a float32 tensor")
        if tuple(weights.shape) != (groups.n_entries,):
            raise ValueError("%s weights for %d entries" % (tuple(weights.shape), groups.n_entries))
        weights = weights.to(bank.device)
    err = bank._err_word()
    kw = dict(rows=groups.rows, weights=weights, normalize=bool(normalize), n_entries=groups.n_entries, err=err)
    if bank.dtype == "fp8":
        total, wsum, count = ops.bank_pool_fp8(bank.codes, bank.exponents, groups.starts, **kw)
    else:
        total, wsum, count = ops.bank_pool(bank.features, groups.starts, **kw)
    bank._checked(err)
    return Descriptors(total, wsum, count, groups.shape)


def describe_scenes(bank, normalize=True):
    """One descriptor per scene of the bank (room type: score ``.queries()`` against a prompt set)."""
    return pool(bank, PointGroups.from_scenes(bank), normalize=normalize)


def describe_objects(result, bank, heat=None):
    """Descriptors [S, Q, M] of the kept objects of a ``find_objects(..., return_point_ids=True)`` result over the bank
    the heat-map came from.  heat (fp16 [N, Q], the searched heat-map): a hit's weight is max(score, 0) of its own query's
    column, else every hit weighs 1."""
    groups = PointGroups.from_objects(result)
    weights = None
    if heat is not None:
        if not isinstance(heat, torch.Tensor) or heat.dim() != 2 or tuple(heat.shape) != tuple(result.point_object.shape):
            raise ValueError("heat must be the [N, Q] heat-map the objects were found in")
        weights = heat[groups.rows.to(heat.device), groups.query.to(heat.device)].float().clamp(min=0).to(groups.device)
    return pool(bank, groups, weights=weights)
