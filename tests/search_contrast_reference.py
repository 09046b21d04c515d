"""What the search with negative queries is held to, and CPU stand-ins for its two kernels (tests/test_search_contrast_cpu.py).

The expected relevancy is built from the plain search alone: the heat-map of cat([queries, negatives]) is split into the
fp16 scores s [N, Q] and g [N, M], and
    nmax = max_i g_i (NaN if one is),   z = (s - nmax) / float32(temperature),   rel = fp16(1 / (1 + exp(-z)))
is evaluated in float64 and rounded to fp16 once (numpy's float64 -> float16 conversion rounds once; torch's goes through
float32)."""
import numpy as np
import torch

import search_fp8_reference as f8
import search_reference as sr


def relevancy_f64(s, g, temperature):
    """fp16 [N, Q] from the fp16 scores s [N, Q] of the queries and g [N, M] of the negatives."""
    s, g = s.detach().cpu().double(), g.detach().cpu().double()
    tau = float(np.float32(temperature))
    if g.shape[0] == 0:
        return torch.zeros(s.shape, dtype=torch.float16)
    nmax = g.max(dim=1, keepdim=True)[0]                       # (torch.max propagates NaN)
    z = (s - nmax) / tau
    rel = 1.0 / (1.0 + torch.exp(-z))
    return torch.from_numpy(rel.numpy().astype(np.float16))


def expected(search, bank, queries, negatives, temperature, normalize):
    """fp16 [N, Q] (CPU): the relevancy the plain `search` of the same bank implies."""
    q = queries.shape[0]
    heat = search(bank, torch.cat([queries, negatives]), k=1, normalize=normalize, return_heat=True).heat
    return relevancy_f64(heat[:, :q], heat[:, q:], temperature)


def ulp_distance(a, b):
    """int64 tensor: distance of two fp16 tensors in units of the last place, as bit patterns on the number line (-0 = +0);
    -1 where exactly one of the two is NaN, 0 where both are."""
    def line(x):
        bits = x.detach().cpu().contiguous().view(torch.int16).long() & 0xFFFF
        mag = bits & 0x7FFF
        return torch.where(bits >= 0x8000, -mag, mag), mag > 0x7C00
    ka, na = line(a)
    kb, nb = line(b)
    dist = (ka - kb).abs()
    dist = torch.where(na & nb, torch.zeros_like(dist), dist)
    return torch.where(na ^ nb, torch.full_like(dist, -1), dist)


# ---- CPU stand-ins for ops.bank_search / ops.bank_search_fp8 with negatives (host-logic tests only)
def _contrast(plain, bank_args, scene_offsets, queries, k, thresholds, normalize, want_heat, negatives, temperature):
    if negatives is None:
        return plain(*bank_args, scene_offsets, queries, k, thresholds, normalize, want_heat)
    q = queries.shape[0]
    heat = plain(*bank_args, scene_offsets, torch.cat([queries, negatives]), k, None, normalize, True)[0]
    rel = relevancy_f64(heat[:, :q], heat[:, q:], temperature)
    top_s, top_p, counts = sr.select(rel, scene_offsets.tolist(), k, thresholds)
    return (rel if want_heat else None), top_s, top_p, counts


def bank_search(bank, scene_offsets, queries, k=16, thresholds=None, normalize=True, want_heat=False, max_scene_rows=None, err=None,
                negatives=None, temperature=0.1):
    return _contrast(sr.bank_search, (bank,), scene_offsets, queries, k, thresholds, normalize, want_heat, negatives, temperature)


def bank_search_fp8(codes, exps, scene_offsets, queries, k=16, thresholds=None, normalize=True, want_heat=False, max_scene_rows=None,
                    err=None, negatives=None, temperature=0.1):
    return _contrast(f8.bank_search_fp8, (codes, exps), scene_offsets, queries, k, thresholds, normalize, want_heat, negatives,
                     temperature)
