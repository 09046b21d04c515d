"""The two-bank search's definitions (include/openscene_amd.h beside osn_bank_search_ensemble) in torch, composed from the plain
and the contrast search of each bank, and CPU stand-ins for its two kernels (tests/test_search_ensemble_cpu.py).

    s_X   the fp16 heat-map the plain search of bank X writes under the caller's normalize;  n_X  the same with normalize=True
    r_X   with negatives, the relevancy map the contrast search of bank X writes;            x_X = s_X, or r_X with negatives
    vocabulary   source(p) = max_q n_A(p, q) < max_q n_B(p, q)   (torch.max propagates NaN; < is IEEE: ties and NaN give A)
                 heat(p, :) = x_B(p, :) where source(p), else x_A(p, :)
    query        source(p, q) = x_A(p, q) < x_B(p, q);  heat(p, q) = x_B(p, q) where source(p, q), else x_A(p, q)
Selection and counts: search_reference.select on that heat-map."""
import numpy as np
import torch

import search_bounds as sb
import search_contrast_reference as cr
import search_fp8_reference as f8
import search_reference as sr

MODES = ("vocabulary", "query")


def pick(mode, n_a, n_b, x_a, x_b):
    """(heat fp16 like x_a, source bool [N] or [N, Q]) from the two banks' heat-maps: n_* the normalised plain scores (used by
    "vocabulary" only), x_* the maps the result is taken from."""
    if mode == "vocabulary":
        source = n_a.float().max(dim=1)[0] < n_b.float().max(dim=1)[0]
        return torch.where(source[:, None], x_b, x_a), source
    assert mode == "query"
    source = x_a.float() < x_b.float()
    return torch.where(source, x_b, x_a), source


def compose(search, bank_a, bank_b, queries, mode, normalize=True, negatives=None, temperature=0.1):
    """(heat, source) the definitions give on the results of `search` (openscene_amd.search.search) of each bank alone."""
    kw = dict(k=1, return_heat=True)
    x_a = search(bank_a, queries, normalize=normalize, negatives=negatives, temperature=temperature, **kw).heat
    x_b = search(bank_b, queries, normalize=normalize, negatives=negatives, temperature=temperature, **kw).heat
    if mode == "vocabulary" and (negatives is not None or not normalize):
        n_a = search(bank_a, queries, normalize=True, **kw).heat
        n_b = search(bank_b, queries, normalize=True, **kw).heat
    else:
        n_a, n_b = x_a, x_b
    return pick(mode, n_a, n_b, x_a, x_b)


# ---- the float64 contract of the pick: where the score intervals of search_bounds decide it
def decided(mode, ref_a, ref_b):
    """(must_be_b, must_be_a) bool numpy arrays, [n] or [n, q], from search_bounds.interval of the stored values of A and B (for
    "vocabulary": with normalize=True): B where every value A can take lies below every value B can take, A where no value of
    A lies below any of B's.  Rows with a NaN end are left undecided here (the planted-row tests hold them exactly)."""
    lo_a, hi_a, lo_b, hi_b = (x.astype(np.float64) for x in (ref_a.lo, ref_a.hi, ref_b.lo, ref_b.hi))
    if mode == "vocabulary":
        lo_a, hi_a, lo_b, hi_b = lo_a.max(1), hi_a.max(1), lo_b.max(1), hi_b.max(1)      # (np.max propagates NaN)
    with np.errstate(invalid="ignore"):
        return hi_a < lo_b, lo_a >= hi_b


def undecided_share(mode, ref_a, ref_b):
    b, a = decided(mode, ref_a, ref_b)
    return 1.0 - float((a | b).mean())


def stored_values(rows, kind):
    """float64 numpy [n, d]: what a bank of `kind` stores for the float32 rows (search_bounds.values of a right append)."""
    if kind == "fp16":
        return sb.values(sb.Stored("fp16", rows.half(), None, None))
    return sb.values(sb.Stored("fp8", None, *f8.quantize(rows)))


# ---- CPU stand-ins for ops.bank_search_ensemble / ops.bank_search_ensemble_fp8 (host-logic tests only)
def _ensemble(plain, args_a, args_b, scene_offsets, queries, k, thresholds, normalize, want_heat, negatives, temperature, mode,
              want_source):
    if mode not in MODES:
        raise ValueError('ensemble_mode must be "vocabulary" or "query" (got %r)' % (mode,))

    def heat_of(args, nrm, neg):
        return plain(*args, scene_offsets, queries, k=1, normalize=nrm, want_heat=True, negatives=neg, temperature=temperature)[0]
    x_a, x_b = heat_of(args_a, normalize, negatives), heat_of(args_b, normalize, negatives)
    n_a, n_b = heat_of(args_a, True, None), heat_of(args_b, True, None)
    heat, source = pick(mode, n_a, n_b, x_a, x_b)
    top_s, top_p, counts = sr.select(heat, scene_offsets.tolist(), k, thresholds)
    if mode == "query" and not want_source:
        source = None
    return (heat if want_heat else None), top_s, top_p, counts, source


def bank_search_ensemble(bank, other, scene_offsets, queries, k=16, thresholds=None, normalize=True, want_heat=False,
                         max_scene_rows=None, err=None, negatives=None, temperature=0.1, mode="vocabulary", want_source=True):
    return _ensemble(cr.bank_search, (bank,), (other,), scene_offsets, queries, k, thresholds, normalize, want_heat, negatives,
                     temperature, mode, want_source)


def bank_search_ensemble_fp8(codes, exps, other_codes, other_exps, scene_offsets, queries, k=16, thresholds=None, normalize=True,
                             want_heat=False, max_scene_rows=None, err=None, negatives=None, temperature=0.1, mode="vocabulary",
                             want_source=True):
    return _ensemble(cr.bank_search_fp8, (codes, exps), (other_codes, other_exps), scene_offsets, queries, k, thresholds, normalize,
                     want_heat, negatives, temperature, mode, want_source)
