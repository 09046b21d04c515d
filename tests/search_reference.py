"""Torch formulas the search tests compare against, and CPU stand-ins for the two kernels (tests/test_search_cpu.py).

Scores: the reference's own expressions, restated:
    normalize   run/evaluate.py:305,310   (hf / (hf.norm(dim=-1, keepdim=True) + 1e-5)).half() @ t.t()
    raw         run/evaluate.py:291       h @ t.t()
Selection: a stable sort by descending score, then index, NaN last."""
import torch


def scores_f64(h, t, normalize, round_normalised=False):
    """float64 evaluation on the stored fp16 rows `h` [N, d] and fp16 queries `t` [Q, d].  round_normalised: keep the
    reference's rounding of the normalised vector to fp16 (the kernel divides after the contraction instead)."""
    hf = h.double()
    if normalize:
        hf = hf / (hf.norm(dim=-1, keepdim=True) + 1e-5)
        if round_normalised:
            hf = hf.half().double()
    return hf @ t.double().t()


def select(heat, offsets, k, thresholds=None):
    """(topk_scores fp16 [S, Q, k], topk_points int64 [S, Q, k], counts int64 [S, Q] or None) from a heat-map [N, Q]."""
    s_n, q_n = len(offsets) - 1, heat.shape[1]
    dev = heat.device
    top_s = torch.full((s_n, q_n, k), float("-inf"), dtype=torch.float16, device=dev)
    top_p = torch.full((s_n, q_n, k), -1, dtype=torch.int64, device=dev)
    counts = torch.zeros((s_n, q_n), dtype=torch.int64, device=dev) if thresholds is not None else None
    for s in range(s_n):
        a, b = int(offsets[s]), int(offsets[s + 1])
        if b == a:
            continue
        block = heat[a:b]
        for q in range(q_n):
            col = block[:, q]
            colf = col.float()
            nan = torch.isnan(colf)
            key = torch.where(nan, torch.full_like(colf, float("-inf")), colf)
            order = torch.sort(key, descending=True, stable=True)[1]          # equal scores (-0 == +0) stay in index order
            order = order[torch.sort(nan[order].to(torch.int8), stable=True)[1]]   # NaN last, in index order
            top = order[:k]
            top_s[s, q, :top.shape[0]] = col[top]
            top_p[s, q, :top.shape[0]] = top
            if counts is not None:
                counts[s, q] = (colf >= thresholds[q]).sum()
    return top_s, top_p, counts


def same_bits(a, b):
    """fp16 tensors equal bit for bit (NaN == NaN, -0 != +0)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ---- inputs and the selection check the GPU search tests share
def unit_rows(n, d, gen, lo=0.5, hi=2.0):
    """unit rows scaled over U(lo, hi) (SURVEY.md 8(d)'s query input): |row . unit query| < 2"""
    x = torch.nn.functional.normalize(torch.randn(n, d, generator=gen), dim=1)
    return x * (lo + (hi - lo) * torch.rand(n, 1, generator=gen))


def text(q, d, gen):
    return torch.nn.functional.normalize(torch.randn(q, d, generator=gen), dim=1).half()


def check_selection(res, heat, offsets, k, thresholds=None):
    """`res` (a SearchResult) holds exactly the selection of `heat`, the kernel's own heat-map"""
    top_s, top_p, counts = select(heat, offsets, k, thresholds)
    assert torch.equal(res.topk_points, top_p)
    assert same_bits(res.topk_scores, top_s)
    if thresholds is not None:
        assert torch.equal(res.counts, counts)


# ---- CPU stand-ins for ops.bank_append / ops.bank_check / ops.bank_search (host-logic tests only)
def bank_append(bank, row0, feats, err, gather=None):
    idx = torch.arange(feats.shape[0]) if gather is None else gather.long()
    ok = (idx >= 0) & (idx < feats.shape[0])
    if not bool(ok.all()):
        err |= 1
    dst = torch.arange(idx.shape[0])[ok] + int(row0)
    bank[dst] = feats[idx[ok]].half()
    return idx.shape[0]


def bank_check(err):
    if int(err.item()) != 0:
        raise RuntimeError("osn_bank_check failed (-1): bank error bits %d" % int(err.item()))


def bank_search(bank, scene_offsets, queries, k=16, thresholds=None, normalize=True, want_heat=False, max_scene_rows=None, err=None):
    hf = bank.float()
    if normalize:
        hf = hf / (hf.norm(dim=-1, keepdim=True) + 1e-5)
    heat = (hf @ queries.float().t()).half()
    top_s, top_p, counts = select(heat, scene_offsets.tolist(), k, thresholds)
    return (heat if want_heat else None), top_s, top_p, counts
