"""Bank points matched to exemplars: for each of L bank rows the k most similar of M exemplar rows, M from a thousand to a
few hundred thousand -- what one annotated or otherwise interesting scan is used for next:

    unit_rows         bank (+ rows) -> fp16 [M, dim]: the rows as the query scores them, bit for bit the Gram matrix's operands
    Exemplars         the prepared image of a row list, its source rows and optional int64 labels; .from_scene
    match             bank x Exemplars -> Matches(idx, score, count): the k best exemplars per row; .rows, .vote
    transfer_labels   label by example: a nearest-neighbour classifier in feature space, with a score floor
    novelty           1 - best score per row: what looks like nothing in the exemplars
    mutual            the pairs that are each other's best, from two k = 1 results: correspondences

The rows are taken as ``(hf / (hf.norm(dim=-1, keepdim=True) + 1e-5)).half()`` (``run/evaluate.py:305,310``) or as they are
stored (normalize=False); the score is their fp16 MFMA product accumulated in fp32; equal scores go to the lower exemplar
position and a NaN ranks last (include/openscene_amd.h states the contract).  The query bank and the exemplars' bank may be
different banks of different kinds, of the same dim.

Kernels: csrc/match.hip through ops.bank_unit_rows / ops.bank_match and their _fp8 twins (an fp8 bank is never
dequantised on the query side; exemplars are widened once); ops.knn_vote for the vote.  No L x M array is made: the
workspace is 8 * L * k * splits bytes.  No CPU path.
"""
import torch

from . import ops
from .search import FeatureBank


def _bank(bank, what="bank"):
    if not isinstance(bank, FeatureBank):
        raise TypeError("%s must be a FeatureBank" % what)
    if bank.dim > ops.BANK_POOL_MAX_DIM:
        raise ValueError("rows of up to %d features can be matched (the bank has %d)" % (ops.BANK_POOL_MAX_DIM, bank.dim))
    return bank


def _row_list(bank, rows):
    if rows is None:
        return None
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int64:
        raise TypeError("rows must be an int64 tensor (or None: every row of the bank)")
    if rows.dim() != 1:
        raise ValueError("rows must be an int64 [L] vector (got %s)" % (tuple(rows.shape),))
    if rows.device != bank.device:
        raise ValueError("rows must be on the bank's device (%s, got %s)" % (bank.device, rows.device))
    return rows.contiguous()


def unit_rows(bank, rows=None, normalize=True):
    """fp16 [M, dim] on the bank's device: the operands of the bank rows `rows` (int64 [M] on the device; None: every row).
    A row outside the bank raises (``ops.bank_check``) and leaves the bank usable.  Synchronises once."""
    _bank(bank)
    rows = _row_list(bank, rows)
    err = bank._err_word()
    if bank.dtype == "fp8":
        out = ops.bank_unit_rows_fp8(bank.codes, bank.exponents, rows, normalize=bool(normalize), err=err)
    else:
        out = ops.bank_unit_rows(bank.features, rows, normalize=bool(normalize), err=err)
    bank._checked(err)
    return out


class Exemplars:
    """A prepared exemplar set: image fp16 [M, dim] (``unit_rows`` of the source rows), rows int64 [M] (the source rows in
    `bank`), labels int64 [M] or None, normalize (how the rows were taken; a match takes its query rows the same way)."""

    def __init__(self, bank, rows=None, labels=None, normalize=True):
        _bank(bank)
        rows = _row_list(bank, rows)
        self.normalize = bool(normalize)
        self.image = unit_rows(bank, rows, self.normalize)
        self.rows = rows if rows is not None else torch.arange(bank.rows, dtype=torch.int64, device=bank.device)
        m = self.image.shape[0]
        if m < 1:
            raise ValueError("at least one exemplar is needed")
        if labels is not None:
            if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64:
                raise TypeError("labels must be an int64 tensor")
            if tuple(labels.shape) != (m,):
                raise ValueError("labels must be an int64 [%d] vector (got %s)" % (m, tuple(labels.shape)))
            labels = labels.to(bank.device).contiguous()
        self.labels = labels

    @classmethod
    def from_scene(cls, bank, which, labels=None, normalize=True):
        """Every row of one scene of `bank` (by name or position) as exemplars; labels int64 [the scene's rows] or None."""
        _bank(bank)
        i = bank.names.index(which) if isinstance(which, str) else int(which)
        if not 0 <= i < len(bank):
            raise IndexError("scene %d of %d" % (i, len(bank)))
        rows = torch.arange(bank.offsets[i], bank.offsets[i + 1], dtype=torch.int64, device=bank.device)
        return cls(bank, rows, labels, normalize)

    def __len__(self):
        return self.image.shape[0]

    @property
    def dim(self):
        return self.image.shape[1]

    @property
    def device(self):
        return self.image.device


class Matches:
    """What `match` returns: idx int32 [L, k] (positions in the exemplar list, -1 past count), score float32 [L, k] (-inf past
    count), count int32 [L], exemplars; a row's list is in descending order of (score, then lower position)."""

    def __init__(self, idx, score, count, exemplars):
        self.idx = idx
        self.score = score
        self.count = count
        self.exemplars = exemplars

    @property
    def k(self):
        return self.idx.shape[1]

    @property
    def rows(self):
        """int64 [L, k]: the rows of the exemplars' bank that were matched, -1 past count."""
        found = self.idx >= 0
        return torch.where(found, self.exemplars.rows[self.idx.clamp(min=0).long()], torch.full_like(self.idx, -1, dtype=torch.int64))

    def vote(self, labels=None, fill=-1):
        """int64 [L]: the label most of a row's k matches hold (``ops.knn_vote``): a tie goes to the label whose first holder
        is the most similar; negative labels are ignored; `fill` without a labelled match.  labels: int64 [M], by default the
        exemplars' own."""
        labels = self.exemplars.labels if labels is None else labels
        if labels is None:
            raise ValueError("the exemplars carry no labels: pass labels")
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64:
            raise TypeError("labels must be an int64 tensor")
        if tuple(labels.shape) != (len(self.exemplars),):
            raise ValueError("labels must be an int64 [%d] vector (got %s)" % (len(self.exemplars), tuple(labels.shape)))
        return ops.knn_vote(labels.to(self.idx.device).contiguous(), self.idx, self.count, fill=fill)


def match(bank, exemplars, k=1, rows=None, splits=None):
    """For each of the bank rows `rows` (int64 [L] on the device; None: every row) the k <= ops.BANK_MATCH_MAX_K most
    similar exemplars -> Matches.  The bank may be another one than the exemplars', of either kind, of the same dim.  A row
    outside the bank raises (``ops.bank_check``) and leaves the bank usable.  `splits` forces how the exemplars are cut over
    workgroups (the result does not depend on it).  Synchronises once."""
    _bank(bank)
    if not isinstance(exemplars, Exemplars):
        raise TypeError("exemplars must be an Exemplars")
    if exemplars.dim != bank.dim:
        raise ValueError("the exemplars have %d features, the bank %d" % (exemplars.dim, bank.dim))
    if exemplars.device != bank.device:
        raise ValueError("the exemplars must be on the bank's device (%s, got %s)" % (bank.device, exemplars.device))
    k = int(k)
    if not 1 <= k <= ops.BANK_MATCH_MAX_K:
        raise ValueError("k must be in 1 .. %d (got %d)" % (ops.BANK_MATCH_MAX_K, k))
    rows = _row_list(bank, rows)
    err = bank._err_word()
    kw = dict(k=k, rows=rows, normalize=exemplars.normalize, splits=splits, err=err)
    if bank.dtype == "fp8":
        idx, score, count = ops.bank_match_fp8(bank.codes, bank.exponents, exemplars.image, **kw)
    else:
        idx, score, count = ops.bank_match(bank.features, exemplars.image, **kw)
    bank._checked(err)
    return Matches(idx, score, count, exemplars)


def transfer_labels(bank, exemplars, k=1, rows=None, min_score=None, fill=-1):
    """int64 [L]: label by example -- the vote of every row's k best exemplars (`Matches.vote`), `fill` where the best
    score is below `min_score` (or NaN) or no match is labelled."""
    m = match(bank, exemplars, k=k, rows=rows)
    out = m.vote(fill=fill)
    if min_score is not None:
        out = torch.where(m.score[:, 0] >= float(min_score), out, torch.full_like(out, int(fill)))
    return out


def novelty(bank, exemplars, rows=None):
    """float32 [L]: 1 - the best score of every row among the exemplars -- 0 for a row the exemplars hold, towards 1 (and
    beyond) for what looks like nothing in them."""
    return 1.0 - match(bank, exemplars, k=1, rows=rows).score[:, 0]


def mutual(matches_ab, matches_ba):
    """The pairs that are each other's best, from two k = 1 results: `matches_ab` of A's rows against exemplars B (one
    exemplar per row of B's query list, in its order) and `matches_ba` the other way round.
    -> int64 [P, 2]: (row of A's list, row of B's list), ascending in the first."""
    if not isinstance(matches_ab, Matches) or not isinstance(matches_ba, Matches):
        raise TypeError("mutual takes two Matches")
    if matches_ab.k != 1 or matches_ba.k != 1:
        raise ValueError("mutual takes two k = 1 results (got k = %d and %d)" % (matches_ab.k, matches_ba.k))
    ab, ba = matches_ab.idx[:, 0].long(), matches_ba.idx[:, 0].long()
    if len(matches_ab.exemplars) != ba.shape[0] or len(matches_ba.exemplars) != ab.shape[0]:
        raise ValueError("the two results do not face each other: %d rows against %d exemplars, %d rows against %d"
                         % (ab.shape[0], len(matches_ab.exemplars), ba.shape[0], len(matches_ba.exemplars)))
    a = torch.arange(ab.shape[0], dtype=torch.int64, device=ab.device)
    back = torch.where(ab >= 0, ba[ab.clamp(min=0)], torch.full_like(ab, -1))
    keep = back == a
    return torch.stack([a[keep], ab[keep]], dim=1)
